"""The training attention core on the 16-bit MFMA (csrc/train_attn16.hip; ``train_block.attention_precision("bf16")``) against the fp32 mode of the same run,
which is the code as it was before the switch existed.  One JSON line per figure (append them to profiles/attn16_bench.jsonl).

  (a) attention_forms     12 heads, 20 views x 768 queries, in the update form (causal prefixes over 15360 memory rows) and the render form (every view over all
                          15360 rows): forward and backward, the two modes alternated round by round in one process on the same tensors; then one profiled
                          round per mode (torch.profiler) for the time of each of the three kernels, their ratios, and the fraction of the matrix peak each
                          reaches (the useful products of the valid (query, key) pairs: 2 per pair in the forward, 4 in dK dV, 3 in dQ, 2 x 64 flop each).
  (b) fp32_vs_other       with ``--other-lib``: the fp32 mode of this build against another build of the library (the parent commit's) on the same tensors,
                          interleaved in the same process: outputs bit-equal, times within the spread.
  (c) decoder_step        figure (b) of scripts/bench_linear16.py -- one scene of 10 views of 768 tokens at the released decoder geometry, schedule [2, 1 x 8]
                          plus a render of all 10 views, forward + backward -- in three settings alternated round by round: fp32, ``linear_precision("bf16")``
                          alone, ``amp("bf16")``; then one profiled pass per setting for the share of the attention kernels.

Timings: ``warmup`` rounds, then ``rounds`` rounds: median, min and max.  "faster" means a gap of the medians larger than the two min-max spreads.  Clocks are
not pinned and the machine is shared: the record says so.
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import decoder_ref as DF  # noqa: E402
from bench_dropout_grad import _attention_case, _library  # noqa: E402
from bench_linear16 import _stats, _verdict  # noqa: E402
from must3r_amd import _lib, train_attention as TA, train_block as TB, train_decoder as TD  # noqa: E402

DEV = "cuda:0"
CONDITIONS = "clocks not pinned, shared machine; wall time around synchronised calls, medians; the settings alternated round by round in one process"
HEADS = 12
PEAK_TFLOPS = {"fp32": 157.3, "bf16": 16 * 157.3}          # dense matrix peaks of the two MFMA pipes
KERNELS = ("attn_fwd", "attn_dkv", "attn_dq")
PRODUCTS = {"attn_fwd": 2, "attn_dkv": 4, "attn_dq": 3}     # matrix products per valid (query, key) pair


def _alternate(fns, settings, rounds, warmup):
    """{setting: {name: [ms]}}: every round times every setting, one after the other"""
    out = {m: {n: [] for n in fns} for m in settings}
    for r in range(warmup + rounds):
        for m, ctx in settings.items():
            with ctx():
                for n, fn in fns.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r >= warmup:
                        out[m][n].append((time.perf_counter() - t0) * 1e3)
    return out


def _kernel_us(fn):
    """{kernel name fragment: GPU microseconds} of the attention kernels of one profiled call, and the total of all kernels"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    by, total = {}, 0.0
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and e.device_time > 0:
            total += e.device_time
            for k in KERNELS:
                if k in e.name:
                    by[k] = by.get(k, 0.0) + e.device_time
    return by, total


def _valid_pairs(tab):
    n = 0
    for q0, nq, k0, nk, lo, hi in tab.tolist():
        n += nq * (nk - (hi - lo))
    return n


MODES = {"fp32": lambda: TB.attention_precision("fp32"), "bf16": lambda: TB.attention_precision("bf16")}


def bench_attention_forms(args):
    g = torch.Generator(device=DEV).manual_seed(0)
    recs = []
    for form in ("update", "render"):
        q, k, v, dO, tab, _ = _attention_case(form, g)
        pairs = _valid_pairs(tab)
        rec = dict(figure="attention_forms", form=form, heads=HEADS, views=20, queries=768, key_rows=int(k.shape[0]), valid_pairs_per_head=pairs,
                   conditions=CONDITIONS)
        fns = dict(forward=lambda: TA.attention_forward(q, k, v, tab, HEADS), backward=lambda: TA.attention_grad(q, k, v, dO, tab, HEADS))
        t = _alternate(fns, MODES, args.rounds, args.warmup)
        for n in fns:
            f32, b16 = _stats(t["fp32"][n], unit="ms"), _stats(t["bf16"][n], unit="ms")
            rec[n] = dict(fp32_ms=f32, bf16_ms=b16, fp32_over_bf16_median=f32["median"] / b16["median"], verdict=_verdict(b16, f32))
        outs = {}
        for m, ctx in MODES.items():
            with ctx():
                outs[m] = [TA.attention_forward(q, k, v, tab, HEADS), *TA.attention_grad(q, k, v, dO, tab, HEADS)]
                try:
                    fwd, _ = _kernel_us(fns["forward"])
                    bwd, _ = _kernel_us(fns["backward"])
                    ks = {"attn_fwd": fwd.get("attn_fwd"), "attn_fwd (statistics pass of the backward)": bwd.get("attn_fwd"), "attn_dkv": bwd.get("attn_dkv"),
                          "attn_dq": bwd.get("attn_dq")}
                    rec[f"{m}_kernels"] = {n: dict(us=us, tflops=PRODUCTS[n.split(" ")[0]] * 2 * 64 * pairs * HEADS / us / 1e6,
                                                   fraction_of_peak=PRODUCTS[n.split(" ")[0]] * 2 * 64 * pairs * HEADS / us / 1e6 / PEAK_TFLOPS[m])
                                           for n, us in ks.items() if us}
                except Exception as e:                # said, not hidden
                    rec[f"{m}_kernels"] = dict(failed=str(e)[:200])
        if all("failed" not in rec[f"{m}_kernels"] for m in MODES):
            rec["kernel_fp32_over_bf16"] = {n: rec["fp32_kernels"][n]["us"] / rec["bf16_kernels"][n]["us"] for n in rec["bf16_kernels"] if n in rec["fp32_kernels"]}
        rec["largest_relative_difference_bf16_vs_fp32"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs["bf16"], outs["fp32"]))
        recs.append(rec)
        del q, k, v, dO, outs
        torch.cuda.empty_cache()
    return recs


def bench_fp32_vs_other(args):
    other = C.CDLL(args.other_lib)
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        if hasattr(other, name):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = restype, argtypes
    mine = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(0)
    recs = []
    for form in ("update", "render"):
        q, k, v, dO, tab, _ = _attention_case(form, g)
        rec = dict(figure="fp32_vs_other", form=form, other=os.path.basename(args.other_lib), heads=HEADS, views=20, queries=768, key_rows=int(k.shape[0]),
                   conditions=CONDITIONS)
        run = lambda: [TA.attention_forward(q, k, v, tab, HEADS), *TA.attention_grad(q, k, v, dO, tab, HEADS)]
        with _library(other):
            ref = run()
        with TB.attention_precision("bf16"):          # toggled before the fp32 run that is compared
            run()
        got = run()
        rec["bit_equal"] = all(torch.equal(a, b) for a, b in zip(got, ref))
        fns = dict(forward=lambda: TA.attention_forward(q, k, v, tab, HEADS), backward=lambda: TA.attention_grad(q, k, v, dO, tab, HEADS))
        t = _alternate(fns, {"this": lambda: _library(mine), "other": lambda: _library(other)}, args.rounds, args.warmup)
        for n in fns:
            a, b = _stats(t["this"][n], unit="ms", what="this build, fp32 mode"), _stats(t["other"][n], unit="ms", what="other build")
            rec[n] = dict(this_ms=a, other_ms=b, other_over_this_median=b["median"] / a["median"], verdict=_verdict(a, b).replace("bf16", "this build"))
        recs.append(rec)
    return recs


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
    settings = {"fp32": contextlib.nullcontext, "linear_bf16": lambda: TB.linear_precision("bf16"), "amp_bf16": lambda: TB.amp("bf16")}
    rec = dict(figure="decoder_step", schedule=[v for v, _ in schedule], render_views=10, tokens=n, Denc=1024, D=768, heads=12, depth=12, feedback="single_mlp",
               memory_mode="norm_y", conditions=CONDITIONS)
    t = _alternate(dict(step=step), settings, args.rounds, args.warmup)
    st = {m: _stats(t[m]["step"], unit="ms") for m in settings}
    rec.update({f"{m}_ms": st[m] for m in settings})
    rec["fp32_over_amp_median"] = st["fp32"]["median"] / st["amp_bf16"]["median"]
    rec["linear_bf16_over_amp_median"] = st["linear_bf16"]["median"] / st["amp_bf16"]["median"]
    rec["verdict_amp_vs_linear_bf16"] = _verdict(st["amp_bf16"], st["linear_bf16"]).replace("bf16 ", "amp ")
    rec["verdict_amp_vs_fp32"] = _verdict(st["amp_bf16"], st["fp32"]).replace("bf16 ", "amp ")
    grads = {}
    for m, ctx in settings.items():
        with ctx():
            step()
            torch.cuda.synchronize()
            grads[m] = {k: p.grad.clone() for k, p in dec.named_parameters()}
            try:
                by, total = _kernel_us(step)
                att = sum(by.values())
                rec[f"{m}_kernel_ms"] = dict(all_kernels=total / 1e3, attention_kernels=att / 1e3, attention_share=att / total if total else None,
                                             by_kernel_ms={k: v / 1e3 for k, v in sorted(by.items())})
            except Exception as e:                # said, not hidden
                rec[f"{m}_kernel_ms"] = dict(failed=str(e)[:200])
    rel = {k: float((grads["amp_bf16"][k] - grads["fp32"][k]).abs().max() / grads["fp32"][k].abs().max()) for k in grads["fp32"]
           if not k.endswith("cross_attn.projk.bias")}
    rec["largest_relative_grad_difference_amp_vs_fp32"] = max(rel.values())
    rec["largest_relative_grad_difference_at"] = max(rel, key=rel.get)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    figures = dict(attention_forms=bench_attention_forms, fp32_vs_other=bench_fp32_vs_other, decoder_step=bench_decoder_step)
    ap.add_argument("--figures", nargs="*", default=["attention_forms", "decoder_step"], choices=list(figures))
    ap.add_argument("--other-lib", default=None, help="another build of libmust3r_hip.so (the parent commit's) for fp32_vs_other")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn16: needs a GPU (no CPU fallback)")
    if "fp32_vs_other" in args.figures and not args.other_lib:
        raise SystemExit("bench_attn16: fp32_vs_other needs --other-lib")
    f = open(args.out, "a") if args.out else None
    for fig in args.figures:
        for rec in figures[fig](args):
            line = json.dumps(rec)
            print(line, flush=True)
            if f:
                f.write(line + "\n")
                f.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
