"""Memory dropout (must3r_amd.train_dropout; the masked kernels of csrc/train_attention.hip) on the GPU.  One JSON line per figure (append them to
profiles/dropout_grad_bench.jsonl).

  (a) masked_attention    the masked attention forward and backward at p = 0.1 against the unmasked call on the same tensors in the same run, at the released
                          geometry: 12 heads, 20 views x 768 queries over 15360 key rows, in the update form (causal prefixes; view j draws over its prefix)
                          and the render form (every view over all rows, one draw shared).  At p = 0.1 no key tile is empty, so nothing is skipped: the
                          verdict is the spread criterion of scripts/bench_decoder_grad.py.
  (b) unmasked_vs_other   with ``--other-lib``: the unmasked entry points of this build against those of another build of the library (the parent commit's)
                          on the same tensors, interleaved in the same process.
  (c) decoder_step        ``train_dropout.CausalMUSt3R(mem_dropout=0.1)`` forward + backward on the schedule of scripts/bench_decoder_grad.py (one scene,
                          [2, 1 x 8] plus a render of 10 views, released geometry) against ``mem_dropout=0`` and against the restated decoder
                          (tests/dropout_ref.py) in fp32 under torch autograd with boolean masks on the same GPU; time and ``max_memory_allocated``.

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared: the record says so.
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_decoder_grad import CONDITIONS, DEV, _stats, _verdict, _wall  # noqa: E402
from must3r_amd import _lib, train_attention as TA, train_decoder as TD, train_dropout as TDO  # noqa: E402

HEADS, VIEWS, N = 12, 20, 768


def _pair(a, b):
    """the verdict's words speak of 'fused' (the first) and 'composed' (the second)"""
    return dict(first_ms=a, second_ms=b, second_over_first_median=b["median"] / a["median"], verdict=_verdict(a, b).replace("fused", "first"))


def _attention_case(form, g):
    D, Rk = HEADS * 64, VIEWS * N
    rn = lambda *s: torch.randn(s, generator=g, device=DEV)
    q, k, v, dO = rn(VIEWS * N, D) * 2.0, rn(Rk, D), rn(Rk, D), rn(VIEWS * N, D) * 1e-7
    if form == "update":
        tab = TA._table(TA.memory_views(1, VIEWS, N, 0, mask=True, causal=True))
        keep = torch.rand((VIEWS, Rk), generator=g, device=DEV) >= 0.1
        view_mask = list(range(VIEWS))
    else:
        tab = TA._table([[j * N, N, 0, Rk, 0, 0] for j in range(VIEWS)])
        keep = torch.rand((1, Rk), generator=g, device=DEV) >= 0.1
        view_mask = [0] * VIEWS
    return q, k, v, dO, tab, TA._mask(TA.pack_key_mask(keep), view_mask, tab, q.device)


def bench_masked_attention(args):
    g = torch.Generator(device=DEV).manual_seed(0)
    recs = []
    for form in ("update", "render"):
        q, k, v, dO, tab, mask = _attention_case(form, g)
        rec = dict(figure="masked_attention", form=form, heads=HEADS, views=VIEWS, queries=N, key_rows=VIEWS * N, p=0.1, conditions=CONDITIONS)
        bits, vm = mask
        words = bits.view(bits.shape[0], -1, 2)
        rec["empty_key_tiles"] = int(((words == 0).all(dim=2)[:, :VIEWS * N // 64]).sum())
        for name, fn in (("forward", lambda m: TA.attention_forward(q, k, v, tab, HEADS, mask=m)),
                         ("backward", lambda m: TA.attention_grad(q, k, v, dO, tab, HEADS, mask=m))):
            # interleaved: unmasked, masked, unmasked, masked ...
            un, ma = [], []
            for _ in range(args.warmup):
                fn(None), fn(mask)
            for _ in range(args.rounds):
                un += _wall(lambda: fn(None), 1, 0)
                ma += _wall(lambda: fn(mask), 1, 0)
            rec[name] = _pair(_stats(un, unit="ms", what="unmasked"), _stats(ma, unit="ms", what="masked"))
        recs.append(rec)
    return recs


@contextlib.contextmanager
def _library(lib):
    keep = _lib._lib
    _lib._lib = lib
    try:
        yield
    finally:
        _lib._lib = keep


def bench_unmasked_vs_other(args):
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
        rec = dict(figure="unmasked_vs_other", form=form, other=os.path.basename(args.other_lib), heads=HEADS, views=VIEWS, queries=N, key_rows=VIEWS * N,
                   conditions=CONDITIONS)
        with _library(other):
            ref = [TA.attention_forward(q, k, v, tab, HEADS), *TA.attention_grad(q, k, v, dO, tab, HEADS)]
        got = [TA.attention_forward(q, k, v, tab, HEADS), *TA.attention_grad(q, k, v, dO, tab, HEADS)]
        rec["bit_equal"] = all(torch.equal(a, b) for a, b in zip(got, ref))
        for name, fn in (("forward", lambda: TA.attention_forward(q, k, v, tab, HEADS)), ("backward", lambda: TA.attention_grad(q, k, v, dO, tab, HEADS))):
            a, b = [], []
            for lib in (mine, other) * args.warmup:
                with _library(lib):
                    fn()
            for _ in range(args.rounds):
                with _library(mine):
                    a += _wall(fn, 1, 0)
                with _library(other):
                    b += _wall(fn, 1, 0)
            rec[name] = _pair(_stats(a, unit="ms", what="this build"), _stats(b, unit="ms", what="other build"))
        recs.append(rec)
    return recs


def bench_decoder_step(args):
    import decoder_ref as DF
    import dropout_ref as DO
    schedule = ((2, False),) + ((1, False),) * 8 + ((10, True),)
    case = DF.make_case(Denc=1024, D=768, heads=12, hidden=3072, depth=12, feedback_type="single_mlp", mode="norm_y", causal=True, scenes=1, grid=(24, 32),
                        seed=5, schedule=schedule)
    n, H, W = case["n"], case["H"], case["W"]
    kw = dict(enc_embed_dim=1024, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, feedback_type="single_mlp", memory_mode="norm_y", protected_imgs=1)
    gen = torch.Generator(device=DEV)
    decs = {"dropout_0": TDO.CausalMUSt3R(mem_dropout=0.0, **kw), "dropout_0.1": TDO.CausalMUSt3R(mem_dropout=0.1, generator=gen, **kw)}
    for d in decs.values():
        d.load_state_dict(case["params"], strict=True)
        d.to(DEV)
    xs = [c["x"].to(DEV).requires_grad_(True) for c in case["calls"]]
    Gs = [c["G"].to(DEV) for c in case["calls"]]
    pos = [case["pos"].to(DEV).view(1, 1, n, 2).expand(1, c["V"], n, 2).contiguous() for c in case["calls"]]
    ts = [torch.tensor([H, W]).view(1, 1, 2).expand(1, c["V"], 2).contiguous() for c in case["calls"]]

    def native(dec):
        def run():
            gen.manual_seed(3)
            dec.zero_grad(set_to_none=True)
            for x in xs:
                x.grad = None
            mem, loss = None, 0
            for c, x, p, t, G in zip(case["calls"], xs, pos, ts, Gs):
                mem, pts = dec(x, p, t, mem, render=c["render"])
                loss = loss + (pts * G).sum()
            loss.backward()
        return run
    rec = dict(figure="decoder_step", schedule=[v for v, _ in schedule], render_views=10, tokens=n, Denc=1024, D=768, heads=12, depth=12, feedback="single_mlp",
               memory_mode="norm_y", dropout_mode="temporary", conditions=CONDITIONS)
    for name, dec in decs.items():
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        native(dec)()
        torch.cuda.synchronize()
        rec[f"{name}_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    a, b = [], []
    for _ in range(args.rounds):
        a += _wall(native(decs["dropout_0"]), 1, 0)
        b += _wall(native(decs["dropout_0.1"]), 1, 0)
    rec["step"] = _pair(_stats(a, unit="ms", what="mem_dropout 0"), _stats(b, unit="ms", what="mem_dropout 0.1"))
    # the reference's method: the restated decoder in fp32 under torch autograd with boolean masks, the draws of the reference's own selector form
    try:
        for d in decs.values():
            d.zero_grad(set_to_none=True)
        sel = TDO.TemporaryMemoryDropoutSelector(0.1)
        state, selections = DO.new_state(), []
        torch.manual_seed(3)
        Nm = 0
        for c in case["calls"]:
            prot = DO.protected_tokens(state, c["V"], n, c["render"])
            selections.append(sel(Nm, 1, 0, protected=prot, device="cpu") if c["render"] else sel(Nm, c["V"], n, protected=prot, device="cpu"))
            if not c["render"]:
                state = dict(state, prot_tokens=prot, prot_imgs=min(1, state["prot_imgs"] + c["V"]))
                Nm += c["V"] * n
        dcase = dict(case, pos=case["pos"].to(DEV))
        leaves = {k: v.to(DEV).requires_grad_(True) for k, v in case["params"].items()}

        def ref():
            for t in (*leaves.values(), *xs):
                t.grad = None
            st, loss = DO.new_state(), 0
            for c, x, s, G in zip(case["calls"], xs, selections, Gs):
                st, _, pts = DO.call(dcase, leaves, x, st, c["render"], s, "temporary")
                loss = loss + (pts * G).sum()
            loss.backward()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        ref()
        torch.cuda.synchronize()
        rec["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        rec["torch_dropout_ref_fp32_ms"] = _stats(_wall(ref, args.torch_rounds, 0), unit="ms")
        rec["speedup_median"] = rec["torch_dropout_ref_fp32_ms"]["median"] / rec["step"]["second_ms"]["median"]
    except Exception as e:                        # e.g. out of memory: said, not hidden
        rec["torch_dropout_ref_fp32_ms"] = dict(failed=str(e)[:200])
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    figures = ["masked_attention", "unmasked_vs_other", "decoder_step"]
    ap.add_argument("--figures", nargs="*", default=["masked_attention", "decoder_step"], choices=figures)
    ap.add_argument("--other-lib", default=None, help="another build of libmust3r_hip.so (the parent commit's) for unmasked_vs_other")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dropout_grad: needs a GPU (no CPU fallback)")
    if "unmasked_vs_other" in args.figures and not args.other_lib:
        raise SystemExit("bench_dropout_grad: unmasked_vs_other needs --other-lib")
    f = open(args.out, "a") if args.out else None
    for fig in args.figures:
        for rec in {"masked_attention": bench_masked_attention, "unmasked_vs_other": bench_unmasked_vs_other, "decoder_step": bench_decoder_step}[fig](args):
            line = json.dumps(rec)
            print(line, flush=True)
            if f:
                f.write(line + "\n")
                f.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
