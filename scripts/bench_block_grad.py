"""The transformer block's training forward and backward (csrc/train_block.hip; must3r_amd.train_block) beside the yardstick's formulas in fp32 under
torch autograd, on the same GPU and the same tensors, in the same run.  One JSON line per shape (append them to profiles/block_grad_bench.jsonl).
Shapes: ``--scenes`` scenes of 20 views of 768 tokens, ``enc`` = D 1024 / 16 heads / hidden 4096 (the encoder's block), ``dec`` = D 768 / 12 heads /
hidden 3072 (the decoder's width).

  (a) the C entry points on preallocated buffers, device events: the four sublayer entry points (every gradient asked for) and the new operators one by
      one -- ``linear_fwd_f32`` in its three epilogues on the block's own Linear shapes, beside ``dgrad_kernel`` on the mirrored shape; ``gelu_grad_f32``,
      ``rope_rows_f32`` and the LayerNorm backward with ``add`` against 6.3 TB/s.
  (b) per launch, from a kernel trace (``--kernel-stats SHAPE=FILE``: the kernel_stats CSV of a separate
      ``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/bench_block_grad.py --kernels-only --shapes S`` run): average time per
      kernel symbol and, for the three ``linear_fwd_f32`` instantiations, the achieved fraction of the 157.3 TFLOP/s fp32 matrix peak.
  (c) forward + backward of ``Block`` under autograd beside tests/block_ref.py in fp32 under torch autograd, and the largest relative difference of the
      gradients (max |a - b| / max |b| per tensor).

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
import block_ref as BR  # noqa: E402
from must3r_amd import _lib, train_block as TB  # noqa: E402
from must3r_amd.train_attention import self_views  # noqa: E402

DEV = "cuda:0"
FP32_MATRIX_FLOPS, HBM_BYTES_PER_S = 157.3e12, 6.3e12
N, V = 768, 20
SHAPES = {"enc": (1024, 16, 4096), "dec": (768, 12, 3072)}


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
    D, heads, hidden = SHAPES[shape]
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, device=DEV)
    M = scenes * V * N
    p = {"norm1.weight": 1 + 0.1 * rn(D), "norm1.bias": 0.1 * rn(D), "attn.qkv.weight": rn(3 * D, D) * D ** -0.5 * 1.5, "attn.qkv.bias": 0.1 * rn(3 * D),
         "attn.proj.weight": rn(D, D) * D ** -0.5, "attn.proj.bias": 0.1 * rn(D), "norm2.weight": 1 + 0.1 * rn(D), "norm2.bias": 0.1 * rn(D),
         "mlp.fc1.weight": rn(hidden, D) * D ** -0.5, "mlp.fc1.bias": 0.1 * rn(hidden), "mlp.fc2.weight": rn(D, hidden) * hidden ** -0.5,
         "mlp.fc2.bias": 0.1 * rn(D)}
    views = self_views(scenes, V, N)
    pos = BR.grid_positions(N, 32).repeat(scenes * V, 1).to(DEV)
    return dict(D=D, heads=heads, hidden=hidden, M=M, x=rn(M, D), dy=rn(M, D) * 1e-7, params=p, views=views, tab=torch.tensor(views, dtype=torch.int32),
                pos=pos, rope_tab=TB.rope_table(DEV))


def flops(t):
    M, D, Hd = t["M"], t["D"], t["hidden"]
    attn_core = sum(4.0 * w[1] * w[3] * 64 for w in t["views"]) * t["heads"]
    lin = lambda n, k: 2.0 * M * n * k
    mlp_f = lin(Hd, D) + lin(D, Hd)
    attn_f = lin(3 * D, D) + lin(D, D) + attn_core
    # backward: the forward once more, then a weight and a data gradient per Linear; the attention core's backward is 1 + 1.5 + 2 forwards
    return dict(mlp_forward=mlp_f, mlp_grad=lin(Hd, D) + 2 * mlp_f, attn_forward=attn_f,
                attn_grad=lin(3 * D, D) + attn_core + 2 * (lin(3 * D, D) + lin(D, D)) + 4.5 * attn_core)


def entry_calls(t):
    """name -> call on preallocated buffers with nothing but the entry point inside"""
    lib = _lib.load()
    M, D, Hd = t["M"], t["D"], t["hidden"]
    stream = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
    mp, ap = [t["params"][k] for k in BR.MLP_PARAMS], [t["params"][k] for k in BR.ATTN_PARAMS]
    nb_m, nb_a = lib.must3r_hip_mlp_sublayer_scratch_bytes(M, D, Hd), lib.must3r_hip_attn_sublayer_scratch_bytes(M, D, len(t["views"]))
    scratch = torch.empty(max(nb_m, nb_a), dtype=torch.uint8, device=DEV)
    out = new(M, D)
    calls, keep = {}, [scratch, out]

    def sub(fn, a, outs, fields, nb):
        keep.extend(outs)
        a.dy, a.out = t["dy"].data_ptr(), out.data_ptr()
        for f, o in zip(fields, outs):
            setattr(a, f, o.data_ptr())
        return lambda: _lib.check(fn(C.byref(a), scratch.data_ptr(), nb, stream))
    calls["mlp_forward"] = sub(lib.must3r_hip_mlp_sublayer_forward, TB._mlp_args(t["x"], *mp, 1e-6), [], [], nb_m)
    calls["mlp_grad"] = sub(lib.must3r_hip_mlp_sublayer_grad, TB._mlp_args(t["x"], *mp, 1e-6), [new(M, D), new(D), new(D), new(Hd, D), new(Hd), new(D, Hd), new(D)],
                            TB.MLP_OUTPUTS, nb_m)
    aa = lambda: TB._attn_args(t["x"], t["pos"], t["tab"], t["rope_tab"], *ap, 1e-6)
    calls["attn_forward"] = sub(lib.must3r_hip_attn_sublayer_forward, aa(), [], [], nb_a)
    calls["attn_grad"] = sub(lib.must3r_hip_attn_sublayer_grad, aa(), [new(M, D), new(D), new(D), new(3 * D, D), new(3 * D), new(D, D), new(D)], TB.ATTN_OUTPUTS, nb_a)
    # the operators one by one
    h, z, qkv = new(M, Hd), new(M, Hd), new(M, 3 * D)
    keep.extend([h, z, qkv])
    P = lambda v: v.data_ptr()
    ops = {}
    lin = lambda epi, A, lda, W, b, res, o, ldc, zz, n, k: (lambda: _lib.check(lib.must3r_hip_op_linear_f32(epi, P(A), lda, P(W), P(b), None if res is None else P(res),
                                                                                                          D, P(o), ldc, None if zz is None else P(zz), n, M, n, k, stream)))
    ops["linear_bias_qkv"] = (lin(_lib.LIN_BIAS, t["x"], D, ap[2], ap[3], None, qkv, 3 * D, None, 3 * D, D), 2.0 * M * 3 * D * D, None)
    ops["linear_bias_gelu_fc1"] = (lin(_lib.LIN_BIAS_GELU, t["x"], D, mp[2], mp[3], None, h, Hd, z, Hd, D), 2.0 * M * Hd * D, None)
    ops["linear_bias_res_fc2"] = (lin(_lib.LIN_BIAS_RES, h, Hd, mp[4], mp[5], t["x"], out, D, None, D, Hd), 2.0 * M * D * Hd, None)
    ops["linear_bias_res_proj"] = (lin(_lib.LIN_BIAS_RES, t["x"], D, ap[4], ap[5], t["x"], out, D, None, D, D), 2.0 * M * D * D, None)
    ops["dgrad_fc1_mirror"] = (lambda: _lib.check(lib.must3r_hip_op_linear_dgrad_f32(P(t["dy"]), D, P(mp[4]), P(h), M, D, Hd, stream)), 2.0 * M * D * Hd, None)
    ops["gelu_grad"] = (lambda: _lib.check(lib.must3r_hip_op_gelu_grad_f32(P(h), Hd, P(z), Hd, P(h), Hd, M, Hd, stream)), None, 3.0 * M * Hd * 4)
    ops["rope_rows"] = (lambda: _lib.check(lib.must3r_hip_op_rope_f32(P(qkv), 3 * D, P(t["pos"]), P(t["rope_tab"]), 256, M, 2 * D, 1, stream)), None, 2.0 * M * 2 * D * 4)
    nb_l = lib.must3r_hip_op_layernorm_grad_scratch_bytes(M, D)
    dx, dg, db = new(M, D), new(D), new(D)
    keep.extend([dx, dg, db])
    ops["layernorm_grad_add"] = (lambda: _lib.check(lib.must3r_hip_op_layernorm_grad_add(P(t["x"]), P(mp[0]), P(t["dy"]), P(t["dy"]), P(dx), P(dg), P(db), M, D, 1e-6,
                                                                                         scratch.data_ptr(), nb_l, stream)), None, 4.0 * M * D * 4)
    ops["layernorm_fwd"] = (lambda: _lib.check(lib.must3r_hip_op_layernorm_f32(P(t["x"]), P(mp[0]), P(mp[1]), P(dx), M, D, 1e-6, stream)), None, 2.0 * M * D * 4)
    return calls, ops, dict(mlp=int(nb_m), attn=int(nb_a)), keep


def bench_entry_points(t, args):
    calls, ops, nbytes, keep = entry_calls(t)
    fl = flops(t)
    out = dict(scratch_bytes=nbytes)
    for name, call in calls.items():
        st = _stats(_events(call, args), unit="ms")
        out[name] = dict(ms=st, flops=fl[name], tflops_of_the_whole_call=fl[name] / (st["median"] * 1e-3) / 1e12,
                         fraction_of_157p3_TFLOPs_whole_call=fl[name] / (st["median"] * 1e-3) / FP32_MATRIX_FLOPS)
    for name, (call, f, b) in ({} if args.kernels_only else ops).items():
        st = _stats(_events(call, args), unit="ms")
        rec = dict(ms=st)
        if f:
            rec.update(flops=f, fraction_of_157p3_TFLOPs=f / (st["median"] * 1e-3) / FP32_MATRIX_FLOPS)
        if b:
            rec.update(bytes=b, fraction_of_6p3_TBps=b / (st["median"] * 1e-3) / HBM_BYTES_PER_S)
        out["op_" + name] = rec
    del keep
    return out


def kernel_rows(path, t):
    """average time per kernel symbol of this file and its two neighbours; the linear_fwd_f32 instantiations also as a fraction of the matrix peak (per sublayer
    forward + backward run, <0> is the qkv Linear twice, <2> fc1 twice, <1> proj and fc2 once each)"""
    M, D, Hd = t["M"], t["D"], t["hidden"]
    per_call = {"linear_fwd_f32<0>": 2.0 * M * 3 * D * D, "linear_fwd_f32<2>": 2.0 * M * Hd * D, "linear_fwd_f32<1>": (2.0 * M * D * D + 2.0 * M * D * Hd) / 2}
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if not any(k in name for k in ("linear_fwd_f32", "ln_fwd_f32", "gelu_grad_f32", "rope_rows_f32", "ln_grad_kernel", "dgrad_kernel", "wgrad_kernel", "attn_")):
                continue
            avg_s = float(r["AverageNs"]) * 1e-9
            row = dict(calls=int(r["Calls"]), avg_ms=avg_s * 1e3, min_ms=float(r["MinNs"]) * 1e-6, max_ms=float(r["MaxNs"]) * 1e-6)
            for k, fl in per_call.items():
                if k in name.replace("(m3r::LinArgs)", ""):
                    row.update(avg_flops=fl, fraction_of_157p3_TFLOPs=fl / avg_s / FP32_MATRIX_FLOPS)
            rows[name[:80]] = row
    return rows


def bench_step(t, args):
    blk = TB.Block(t["D"], t["heads"], t["hidden"] / t["D"]).to(DEV)
    blk.load_state_dict(t["params"])
    leaves = {k: v.clone().requires_grad_(True) for k, v in t["params"].items()}
    x = t["x"].clone().requires_grad_(True)

    def native():
        blk.zero_grad(set_to_none=True)
        x.grad = None
        blk(x, t["pos"], t["views"]).backward(t["dy"])
        return dict(dx=x.grad, **{k: p.grad for k, p in blk.named_parameters()})

    def ref():
        for v in leaves.values():
            v.grad = None
        x.grad = None
        BR.block(x, t["pos"], t["views"], t["heads"], leaves).backward(t["dy"])
        return dict(dx=x.grad, **{k: v.grad for k, v in leaves.items()})
    g_n = {k: v.clone() for k, v in native().items()}
    rec = dict(native_s=_stats(_wall(native, args.rounds, args.warmup), unit="s"))
    try:
        g_t = ref()
        rec["max_relative_grad_difference"] = {k: float((g_n[k] - g_t[k]).abs().max() / g_t[k].abs().max()) for k in g_n}
        rec["largest_relative_grad_difference"] = max(rec["max_relative_grad_difference"].values())
        del g_t
        rec["torch_block_ref_fp32_s"] = _stats(_wall(ref, args.torch_rounds, 1), unit="s")
        rec["speedup_median"] = rec["torch_block_ref_fp32_s"]["median"] / rec["native_s"]["median"]
    except RuntimeError as e:                     # e.g. out of memory: said, not hidden
        rec["torch_block_ref_fp32_s"] = dict(failed=str(e)[:200])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["enc", "dec"], choices=list(SHAPES))
    ap.add_argument("--scenes", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="figure (a) alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="SHAPE=kernel_stats.csv of a --kernels-only run of that shape under rocprofv3: figure (b)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_block_grad: needs a GPU (no CPU fallback)")
    stats = dict(s.split("=", 1) for s in args.kernel_stats)
    f = open(args.out, "a") if args.out else None
    for shape in args.shapes:
        t = make_inputs(shape, args.scenes)
        rec = dict(figure="block_grad", shape=shape, scenes=args.scenes, D=t["D"], heads=t["heads"], hidden=t["hidden"], views=len(t["views"]), tokens=N, rows=t["M"],
                   conditions="clocks not pinned, shared machine; device events around the C entry points on preallocated buffers, medians")
        if shape in stats:
            rec["kernels"] = kernel_rows(stats[shape], t)
        else:
            rec["entry_points"] = bench_entry_points(t, args)
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
