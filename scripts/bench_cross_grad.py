"""The cross-attention sublayer's and CachedDecoderBlock's training forward and backward (csrc/train_cross.hip; must3r_amd.train_cross) beside the
yardstick's formulas (tests/decblock_ref.py) in fp32 under torch autograd, on the same GPU and the same tensors, in the same run.  One JSON line per case
(append them to profiles/cross_grad_bench.jsonl).  One scene of 20 views of 768 tokens at D 768 / 12 heads / hidden 3072, ``norm_y`` memory mode:

  update_nm0       the update form over an empty memory: the key rows are the 20 views' own norm_y rows, a view does not attend itself
  update_nm15360   the update form over 15360 memory rows followed by the 20 views' rows (30720 key rows)
  render           768 queries x 20 views over 15360 memory rows

  (a) the two C entry points on preallocated buffers, device events: the sublayer's forward and its backward with every gradient asked for; scratch bytes.
  (b) the segmented data gradient (dmem = dK Wk + dV Wv, one launch over the two parameters) against ``dgrad_kernel`` on a packed [2 D][D] copy of Wk over Wv
      at the same Rm x 2 D x D, plus the copy's own time.  The segmented launch has no entry point of its own; its time is a difference of three medians:
      the backward asked for dmem alone, minus the same call in the ``kv`` mode on the projected k | v (everything but the K | V projection and the data
      gradient), minus the two projection launches.  The spread (min and max of each term) is recorded beside it.
  (c) forward + backward of ``CachedDecoderBlock`` under autograd (x and the memory are leaves) beside tests/decblock_ref.py in fp32 under torch autograd, and
      the largest relative difference of the gradients (max |a - b| / max |b| per tensor).

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
import block_ref as BR  # noqa: E402
import decblock_ref as DR  # noqa: E402
from must3r_amd import _lib, train_cross as TC  # noqa: E402
from must3r_amd.train_attention import memory_views, self_views  # noqa: E402

DEV = "cuda:0"
FP32_MATRIX_FLOPS = 157.3e12
N, V, D, HEADS, HIDDEN = 768, 20, 768, 12, 3072
CASES = {"update_nm0": 0, "update_nm15360": 15360, "render": 15360}


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


def make_inputs(case, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = {k: v.to(DEV) for k, v in DR.make_params(D, HIDDEN, g).items()}
    gd = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gd, device=DEV)
    Nm, M = CASES[case], V * N
    render = case == "render"
    views = [[j * N, N, 0, Nm, 0, 0] for j in range(V)] if render else memory_views(1, V, N, Nm, mask=True)
    Rm = Nm if render else Nm + M
    return dict(case=case, render=render, M=M, Rm=Rm, Nm=Nm, x=rn(M, D), mem=rn(Nm, D) if Nm else None, keys=rn(Rm, D), dy=rn(M, D) * 1e-7, params=p, views=views,
                tab=torch.tensor(views, dtype=torch.int32), self_views=self_views(1, V, N), pos=BR.grid_positions(N, 32).repeat(V, 1).to(DEV), eps=1e-6,
                mode="norm_y", heads=HEADS, scenes=1, rope=(100.0, 1.0))


def flops(t):
    M, Rm = t["M"], t["Rm"]
    core = sum(4.0 * w[1] * (w[3] - (w[5] - w[4])) * 64 for w in t["views"]) * HEADS
    lin = lambda r: 2.0 * r * D * D
    fwd = 2 * lin(M) + 2 * lin(Rm) + core
    # backward: the projections once more and the attention forward for dWproj, then a weight and a data gradient per Linear (no data gradient through
    # Wproj's input side beyond do); the attention core's backward is 1 + 1.5 + 2 forwards
    return dict(forward=fwd, grad=(lin(M) + 2 * lin(Rm) + core) + 2 * (2 * lin(M) + 2 * lin(Rm)) + 4.5 * core)


def bench_entry_points(t, args):
    lib = _lib.load()
    M, Rm = t["M"], t["Rm"]
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
    pc = [t["params"][k] for k in DR.CROSS_PARAMS]
    nb = lib.must3r_hip_cross_sublayer_scratch_bytes(M, Rm, D, len(t["views"]), 0)
    nb_kv = lib.must3r_hip_cross_sublayer_scratch_bytes(M, Rm, D, len(t["views"]), 1)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out, outs = new(M, D), [new(M, D), new(Rm, D), new(D), new(D), new(D, D), new(D), new(D, D), new(D), new(D, D), new(D), new(D, D), new(D)]

    def desc(mem, kv=False):
        a = TC._cross_args(t["x"], mem, t["tab"], *[None if kv and 4 <= i < 8 else w for i, w in enumerate(pc)], t["eps"])
        a.dy, a.out = t["dy"].data_ptr(), out.data_ptr()
        return a
    rec = dict(scratch_bytes=int(nb), scratch_bytes_kv_mode=int(nb_kv))
    fl = flops(t)
    a = desc(t["keys"])
    call = lambda: _lib.check(lib.must3r_hip_cross_sublayer_forward(C.byref(a), scratch.data_ptr(), nb))
    st = _stats(_events(call, args), unit="ms")
    rec["forward"] = dict(ms=st, flops=fl["forward"], fraction_of_157p3_TFLOPs_whole_call=fl["forward"] / (st["median"] * 1e-3) / FP32_MATRIX_FLOPS)
    b = desc(t["keys"])
    for f, o in zip(TC.CROSS_OUTPUTS, outs):
        setattr(b, f, o.data_ptr())
    b.lddmem = D
    call = lambda: _lib.check(lib.must3r_hip_cross_sublayer_grad(C.byref(b), scratch.data_ptr(), nb))
    st = _stats(_events(call, args), unit="ms")
    rec["grad"] = dict(ms=st, flops=fl["grad"], fraction_of_157p3_TFLOPs_whole_call=fl["grad"] / (st["median"] * 1e-3) / FP32_MATRIX_FLOPS)
    # (b) the segmented data gradient by difference, the packed one directly
    Wk, bk, Wv, bv = pc[4:8]
    kv, dkv = new(Rm, 2 * D), new(Rm, 2 * D)
    stream = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))
    P = lambda v: v.data_ptr()

    def project():
        _lib.check(lib.must3r_hip_op_linear_f32(_lib.LIN_BIAS, P(t["keys"]), D, P(Wk), P(bk), None, 0, P(kv), 2 * D, None, 0, Rm, D, D, stream))
        _lib.check(lib.must3r_hip_op_linear_f32(_lib.LIN_BIAS, P(t["keys"]), D, P(Wv), P(bv), None, 0, P(kv) + 4 * D, 2 * D, None, 0, Rm, D, D, stream))
    c = desc(t["keys"])
    c.dmem, c.lddmem = outs[1].data_ptr(), D
    e = desc(kv, kv=True)
    e.dmem, e.lddmem = dkv.data_ptr(), 2 * D
    project()
    t_tok = _stats(_events(lambda: _lib.check(lib.must3r_hip_cross_sublayer_grad(C.byref(c), scratch.data_ptr(), nb)), args), unit="ms")
    t_kv = _stats(_events(lambda: _lib.check(lib.must3r_hip_cross_sublayer_grad(C.byref(e), scratch.data_ptr(), nb)), args), unit="ms")
    t_proj = _stats(_events(project, args), unit="ms")
    packed_w, packed_out = new(2 * D, D), new(Rm, D)

    def copy():
        packed_w[:D].copy_(Wk)
        packed_w[D:].copy_(Wv)
    t_copy = _stats(_events(copy, args), unit="ms")
    t_packed = _stats(_events(lambda: _lib.check(lib.must3r_hip_op_linear_dgrad_f32(P(dkv), 2 * D, P(packed_w), P(packed_out), Rm, 2 * D, D, stream)), args), unit="ms")
    torch.cuda.synchronize()
    seg = t_tok["median"] - t_kv["median"] - t_proj["median"]
    f = 2.0 * Rm * 2 * D * D
    rec["segmented_dgrad"] = dict(shape=[Rm, 2 * D, D], grad_dmem_only_ms=t_tok, grad_dmem_only_kv_mode_ms=t_kv, kv_projection_ms=t_proj,
                                  segmented_ms_by_difference=seg,
                                  spread_ms=[t_tok["min"] - t_kv["max"] - t_proj["max"], t_tok["max"] - t_kv["min"] - t_proj["min"]],
                                  packed_dgrad_ms=t_packed, packed_copy_ms=t_copy, bit_equal=bool(torch.equal(outs[1], packed_out)),
                                  packed_fraction_of_157p3_TFLOPs=f / (t_packed["median"] * 1e-3) / FP32_MATRIX_FLOPS,
                                  segmented_fraction_of_157p3_TFLOPs=f / (seg * 1e-3) / FP32_MATRIX_FLOPS if seg > 0 else None)
    return rec


def bench_step(t, args):
    blk = TC.CachedDecoderBlock(D, HEADS, HIDDEN / D, "norm_y").to(DEV)
    blk.load_state_dict(t["params"])
    leaves = {k: v.clone().requires_grad_(True) for k, v in t["params"].items()}
    x = t["x"].clone().requires_grad_(True)
    mem = t["mem"].clone().requires_grad_(True) if t["Nm"] else None

    def native():
        blk.zero_grad(set_to_none=True)
        x.grad = None
        if mem is not None:
            mem.grad = None
        y = mem if t["render"] else TC.memory_rows(mem, blk.prepare_y(x), 1)
        blk(x, y, t["pos"], t["self_views"], t["views"]).backward(t["dy"])
        return dict(dx=x.grad, **({} if mem is None else dict(dmem=mem.grad)), **{k: p.grad for k, p in blk.named_parameters() if p.grad is not None})

    def ref():
        for v in leaves.values():
            v.grad = None
        x.grad = None
        if mem is not None:
            mem.grad = None
        new = DR.prepare_y(x, leaves, "norm_y")
        y = mem if t["render"] else (new if mem is None else DR.memory_rows(mem, new, 1))
        DR.block(x, y, t["pos"], t["self_views"], t["views"], HEADS, leaves, "norm_y").backward(t["dy"])
        return dict(dx=x.grad, **({} if mem is None else dict(dmem=mem.grad)), **{k: v.grad for k, v in leaves.items() if v.grad is not None})
    g_n = {k: v.clone() for k, v in native().items()}
    rec = dict(native_s=_stats(_wall(native, args.rounds, args.warmup), unit="s"))
    try:
        g_t = ref()
        # cross_attn.projk.bias: the true gradient is zero where every key carries the bias (both sides hold rounding noise): left out of the ratio
        rel = {k: float((g_n[k] - g_t[k]).abs().max() / g_t[k].abs().max()) for k in g_n if k != "cross_attn.projk.bias"}
        rec["max_relative_grad_difference"] = rel
        rec["largest_relative_grad_difference"] = max(rel.values())
        del g_t
        rec["torch_decblock_ref_fp32_s"] = _stats(_wall(ref, args.torch_rounds, 1), unit="s")
        rec["speedup_median"] = rec["torch_decblock_ref_fp32_s"]["median"] / rec["native_s"]["median"]
    except RuntimeError as e:                     # e.g. out of memory: said, not hidden
        rec["torch_decblock_ref_fp32_s"] = dict(failed=str(e)[:200])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="figures (a) and (b) alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cross_grad: needs a GPU (no CPU fallback)")
    f = open(args.out, "a") if args.out else None
    for case in args.cases:
        t = make_inputs(case)
        rec = dict(figure="cross_grad", case=case, D=D, heads=HEADS, hidden=HIDDEN, views=V, tokens=N, query_rows=t["M"], key_rows=t["Rm"], memory_rows=t["Nm"],
                   conditions="clocks not pinned, shared machine; device events around the C entry points on preallocated buffers, medians")
        rec["entry_points"] = bench_entry_points(t, args)
        if not args.no_step:
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
