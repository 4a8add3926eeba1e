"""GPU (-m gpu): the trainable decoder -- must3r_amd/train_decoder.py on csrc/train_decoder.hip (must3r_hip_feedback_prepare_forward / _grad) -- against the
yardstick tests/decoder_ref.py (itself held to the reference's own MUSt3R and CausalMUSt3R classes by tests/test_decoder_grad_host.py).

The bound is that of the other training tests (tests/grad_parity.py): ``e_gpu <= 4 e_ref + 32 2^-24 m`` against the fp64 yardstick, e_ref the error of the
same formulas under fp32 CPU autograd, m = max|g64| -- with the magnitude exception of tests/test_cross_grad_gpu.py: every key a view sees carries
cross_attn.projk.bias, so the true gradient of that bias is zero, and m is the magnitude of what cancels, max_c sum_r |dK_rc| of the fp64 yardstick over every
tensor of projected keys of the schedule (in the decoder this holds in the ``kv`` mode too: there the memory's keys are this decoder's own projections).
The pointmaps go through the head's split-precision forward and are held to the bound tests/test_head_grad_gpu.py uses for it (rtol 1e-5, atol 1e-4).
Every tensor's row is printed before it is asserted; the worst row of each group of tensors goes, as a table, to the file M3R_DECODER_GRAD_TABLE names
(kept as profiles/decoder_grad_parity.txt).

The decoder's schedule is decoder_ref.SCHEDULE on B = 2 scenes of 5 x 7 token views (see tests/test_decoder_grad_host.py).  The operator's shapes: D 64 / 128 /
1024 (one, two and all four float4 per lane), R = 1, 70 and 19 (the backward's block of 16 rows plus a tail; 19 and 70 are no multiples of the forward's four
rows per block either), L = 1 / 2 / 3 / 12, add_layers L - 1 and 0, with and without norms."""
import ctypes as C
import functools
import os
import time

import pytest
import torch

import decoder_ref as DF
import grad_parity as GP
from must3r_amd import _lib, train_block as TB, train_decoder as TD

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.25e11
KBIAS = "cross_attn.projk.bias"

_HEADER = (
    "# tests/test_decoder_grad_gpu.py: per case and tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in units of",
    "# 2^-24 m; bound = 4 e_ref + 32; ratio = e_gpu / bound.  m = max|g64|, except for cross_attn.projk.bias (every key of a view carries the bias, the",
    "# true gradient is zero): there m = the largest column 1-norm of the fp64 dK over the schedule.  Forward outputs are held to the same bound.",
    "# Every tensor is held to the bound; a row is the worst tensor of its group (operator: over L, R and add_layers, named in brackets; decoder: over",
    "# the calls, the memory's layers or the blocks).",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_DECODER_GRAD_TABLE"), _HEADER, list(_worst.values()), (34, 60), magnitude="m")


def _group(name):
    """tokens0 -> tokens, blocks_dec.2.mlp.fc1.weight -> blocks, y3 -> y, ...: the groups of the table"""
    head = name.split(".")[0]
    return {"blocks_dec": "blocks", "feedback_layer": "feedback", "feedback_norm": "feedback", "norm_dec": "head", "head_dec": "head",
            "feat_embed_enc_to_dec": "embed", "image2_embed": "embed"}.get(head, head.rstrip("0123456789"))


def _compare(tag, got, g64, g32, mags=None, fold=None):
    """grad_parity.compare on every tensor (each one printed and held to the bound); the table keeps, per ``fold`` (the tag by default) and group of
    tensors, the row with the worst ratio, the tensor's name beside the group's."""
    rows = []
    try:
        GP.compare(rows, tag, got, g64, g32, mags)
    finally:
        fold = tag if fold is None else fold
        for r in rows:
            key = (fold, _group(r[1]))
            if key not in _worst or r[5] > _worst[key][5]:
                _worst[key] = (fold, f"{key[1]}: {r[1]}" + ("" if fold == tag else f" [{tag[len(fold):].strip()}]"), *r[2:])


_worst = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) feedback_prepare against the fp64 composed formula
# ---------------------------------------------------------------------------------------------------------------------------------
def _fp_case(L, R, D, norm, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    # rows with their own offset and scale, so that mu and rstd matter
    xs = [rn(R, D) * (0.5 + 2.0 * torch.rand((R, 1), generator=g)) + rn(R, 1) for _ in range(L)]
    return dict(L=L, R=R, D=D, norm=norm, xs=xs, offset=0.5 * rn(R, D), gammas=[1 + 0.1 * rn(D) for _ in range(L)], betas=[0.1 * rn(D) for _ in range(L)],
                dys=[rn(R, D) * 1e-7 for _ in range(L)])


def _fp_grads(c, add_layers, dtype, device="cpu", fn=None):
    """dict y{l}, dx{l}, doffset, dgamma{l}, dbeta{l} by autograd through ``fn`` (the yardstick's formula by default)"""
    leaf = lambda t: t.to(device=device, dtype=dtype).clone().requires_grad_(True)
    xs, off = [leaf(t) for t in c["xs"]], leaf(c["offset"]) if add_layers else None
    gs, bs = ([leaf(t) for t in c["gammas"]], [leaf(t) for t in c["betas"]]) if c["norm"] else (None, None)
    ys = (fn or DF.feedback_prepare)(xs, off, gs, bs, add_layers, 1e-6)
    torch.autograd.backward(ys, [d.to(device=device, dtype=dtype) for d in c["dys"]])
    res = {}
    for l in range(c["L"]):
        res[f"y{l}"], res[f"dx{l}"] = ys[l].detach(), xs[l].grad
        if c["norm"]:
            res[f"dgamma{l}"], res[f"dbeta{l}"] = gs[l].grad, bs[l].grad
    if add_layers:
        res["doffset"] = off.grad
    return res


@pytest.mark.parametrize("D", [64, 128, 1024])
def test_feedback_prepare_matches_the_composed_formula(D):
    for L in (1, 2, 3, 12):
        for R in (1, 19, 70):
            for norm in (True, False):
                c = _fp_case(L, R, D, norm, 1000 * L + R + D)
                for add_layers in sorted({L - 1, 0}):
                    g64, g32 = _fp_grads(c, add_layers, torch.float64), _fp_grads(c, add_layers, torch.float32)
                    got = _fp_grads(c, add_layers, torch.float32, DEV, TD.feedback_prepare)
                    assert set(got) == set(g64)
                    _compare(f"fp D{D} {'ln' if norm else 'raw'} L{L} R{R} a{add_layers}", got, g64, g32, fold=f"fp D{D} {'ln' if norm else 'raw'}")


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) feedback_prepare: bits and structure
# ---------------------------------------------------------------------------------------------------------------------------------
def _fp_dev(c):
    d = dict(c)
    for k in ("xs", "gammas", "betas", "dys"):
        d[k] = [t.to(DEV) for t in c[k]]
    d["offset"] = c["offset"].to(DEV)
    return d


def _fp_direct(d, add_layers, rows=None, **want):
    """both operator forms on (a row range of) the case: (ys, dxs, doffset, dgammas, dbetas)"""
    sl = slice(None) if rows is None else slice(*rows)
    xs, dys, off = [t[sl].contiguous() for t in d["xs"]], [t[sl].contiguous() for t in d["dys"]], d["offset"][sl].contiguous()
    gs, bs = (d["gammas"], d["betas"]) if d["norm"] else (None, None)
    ys = TD.feedback_prepare_forward(xs, off if add_layers else None, gs, bs, add_layers)
    g = TD.feedback_prepare_grad(xs, off if add_layers else None, gs, dys, add_layers, want_doffset=add_layers > 0, **want)
    torch.cuda.synchronize()
    return (ys, *g)


def test_layers_without_the_add_have_the_bits_of_layer_norm():
    for D, R in ((64, 70), (768, 19), (1024, 5)):
        d = _fp_dev(_fp_case(3, R, D, True, 7 + D))
        for add_layers in (2, 0):
            ys = _fp_direct(d, add_layers)[0]
            for l in range(add_layers, 3):
                assert torch.equal(ys[l], TB.layer_norm(d["xs"][l], d["gammas"][l], d["betas"][l], 1e-6)), (D, add_layers, l)
            for l in range(add_layers):      # and a layer with it: the same routine on the sum
                assert torch.equal(ys[l], TB.layer_norm(d["xs"][l] + d["offset"], d["gammas"][l], d["betas"][l], 1e-6)), (D, add_layers, l)


def _flat(outs):
    return [t for o in outs for t in (o if isinstance(o, (list, tuple)) else [o]) if t is not None]


def test_calls_repeat_bitwise_and_a_scene_alone_has_the_batchs_bits():
    for norm in (True, False):
        d = _fp_dev(_fp_case(3, 2 * 35, 128, norm, 11))
        a, b = _fp_direct(d, 2), _fp_direct(d, 2)
        assert len(_flat(a)) == (3 + 3 + 1 + (6 if norm else 0)) and all(torch.equal(s, t) for s, t in zip(_flat(a), _flat(b)))
        for lo, hi in ((0, 35), (35, 70)):
            alone = _fp_direct(d, 2, rows=(lo, hi))
            for l in range(3):
                assert torch.equal(alone[0][l], a[0][l][lo:hi]) and torch.equal(alone[1][l], a[1][l][lo:hi]), (norm, lo, l)
            assert torch.equal(alone[2], a[2][lo:hi])


def test_unrequested_outputs_are_left_untouched():
    """One arena of canaries holds every output of the backward, a guard between each two; only the requested ones are handed to the library."""
    lib = _lib.load()
    L, R, D = 3, 19, 128
    d = _fp_dev(_fp_case(L, R, D, True, 13))
    full = _fp_direct(d, 2)
    slots = [(f"dx{l}", R * D) for l in range(L)] + [("doffset", R * D)] + [(f"dgamma{l}", D) for l in range(L)] + [(f"dbeta{l}", D) for l in range(L)]
    truth = dict(zip([n for n, _ in slots], [*full[1], full[2], *full[3], *full[4]]))
    for asked in ({"dx1"}, {"doffset"}, {"dgamma2", "dbeta0"}, {"dx0", "dx2", "dbeta1"}, set()):
        arena = torch.full((sum(n + 64 for _, n in slots),), CANARY, dtype=torch.float32, device=DEV)
        a = TD._fb_args(d["xs"], d["offset"], d["gammas"], d["gammas"], 2, 1e-6)
        at, where = 64, {}
        for name, n in slots:
            where[name] = (at, at + n)
            at += n + 64
        for l in range(L):
            a.dy[l] = d["dys"][l].data_ptr()
        for name in asked:
            ptr = arena.data_ptr() + 4 * where[name][0]
            if name == "doffset":
                a.doffset = C.c_void_p(ptr)
            else:
                getattr(a, name[:-1])[int(name[-1])] = ptr
        nbytes = lib.must3r_hip_feedback_prepare_scratch_bytes(L, R, D)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.check(lib.must3r_hip_feedback_prepare_grad(C.byref(a), C.c_void_p(scratch.data_ptr()), nbytes))
        torch.cuda.synchronize()
        keep = torch.ones_like(arena, dtype=torch.bool)
        for name in asked:
            lo, hi = where[name]
            assert torch.equal(arena[lo:hi], truth[name].reshape(-1)), (asked, name)
            keep[lo:hi] = False
        assert bool((arena[keep] == CANARY).all()), asked
    # the forward: a layer without an output pointer is skipped
    arena = torch.full((3 * R * D,), CANARY, dtype=torch.float32, device=DEV)
    a = TD._fb_args(d["xs"], d["offset"], d["gammas"], d["betas"], 2, 1e-6)
    a.y[1] = arena.data_ptr() + 4 * R * D
    _lib.check(lib.must3r_hip_feedback_prepare_forward(C.byref(a), None, 0))
    torch.cuda.synchronize()
    assert torch.equal(arena[R * D:2 * R * D], full[0][1].reshape(-1)) and bool((arena[:R * D] == CANARY).all()) and bool((arena[2 * R * D:] == CANARY).all())


def _stream_call(bufs, c):
    """both entry points on the current stream (through _lib.stream_ptr), on the bound input buffers"""
    L = c["L"]
    xs, gs, bs, dys = ([bufs[f"{n}{l}"] for l in range(L)] for n in ("x", "gamma", "beta", "dy"))
    ys = TD.feedback_prepare_forward(xs, bufs["offset"], gs, bs, L - 1)
    dxs, doff, dgs, dbs = TD.feedback_prepare_grad(xs, bufs["offset"], gs, dys, L - 1)
    return [*ys, *dxs, doff, *dgs, *dbs]


def test_both_entry_points_run_on_the_descriptors_stream():
    """The protocol of tests/test_stream_order_gpu.py, as tests/test_cross_grad_gpu.py applies it: reference bits of two input sets A and B on the default
    stream; then, with the inputs holding B, on a side stream the null stream overtakes: a delay, copies of A, the calls with a->stream = the side stream,
    clones of the outputs, B back.  The clones must be A's bits and the delay must still be running when the calls have returned.  Control: the same calls
    with a->stream = NULL reproduce B's bits."""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay, null_stream
    delay = Delay()
    cA, cB = _fp_case(3, 70, 128, True, 21), _fp_case(3, 70, 128, True, 22)

    def flat(c):
        out = {"offset": c["offset"].to(DEV)}
        for l in range(3):
            out.update({f"x{l}": c["xs"][l].to(DEV), f"gamma{l}": c["gammas"][l].to(DEV), f"beta{l}": c["betas"][l].to(DEV), f"dy{l}": c["dys"][l].to(DEV)})
        return out
    src = {"A": flat(cA), "B": flat(cB)}
    bufs = {k: torch.empty_like(v) for k, v in src["A"].items()}

    def load(which):
        for k, v in src[which].items():
            bufs[k].copy_(v)
    ref = {}
    for which in ("A", "A", "B"):
        load(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = _stream_call(bufs, cA)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        ref[which] = [t.clone() for t in outs]
    assert sum(float((a != b).float().mean()) for a, b in zip(ref["A"], ref["B"])) / len(ref["A"]) > 0.5
    ms = min(DELAY_CAP_MS, 30.0 + 10.0 * host_ms)
    assert ms < DELAY_CAP_MS or host_ms < DELAY_CAP_MS / 10
    # the side stream
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")
        t0 = time.perf_counter()
        outs = _stream_call(bufs, cA)
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = [t.clone() for t in outs]
        load("B")
    s.synchronize()
    print(f"feedback_prepare: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the calls took {side_ms:.3f} ms on the host)"
    for i, (g, r) in enumerate(zip(got, ref["A"])):
        assert torch.equal(g, r), f"output {i}: on a side stream the bits differ from the default-stream bits (equal to the decoy's: {torch.equal(g, ref['B'][i])})"
    # the control: a->stream = NULL reads the decoy
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")                         # queued behind the delay: the inputs still hold the decoy
        with null_stream():
            outs = _stream_call(bufs, cA)
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.cuda.default_stream().synchronize()
            got = [t.clone() for t in outs]
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    assert premise, f"the delay ({ms:.1f} ms) ended before the null stream was idle"
    for i, (g, r) in enumerate(zip(got, ref["B"])):
        assert torch.equal(g, r), f"output {i}: with a->stream = NULL the calls did not run on the null stream"


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the decoder over the schedule
# ---------------------------------------------------------------------------------------------------------------------------------
GEOMS = {
    "d64": dict(),                                                                                        # the schedule of the host test
    "d128_linear": dict(D=128, heads=2, hidden=512, depth=2, feedback_type="single_linear", seed=72),
    "d64_nofeedback": dict(depth=2, feedback_type=None, seed=73),
}


@functools.lru_cache(maxsize=None)
def _case(geom, mode, causal):
    return DF.make_case(mode=mode, causal=causal, **GEOMS[geom])


@functools.lru_cache(maxsize=None)
def _reference(geom, mode, causal):
    """(fp64 results, fp32 results, magnitudes): computed once, shared, never modified."""
    extra = {}
    g64 = DF.grads(_case(geom, mode, causal), torch.float64, "pointmaps", extra)
    return g64, DF.grads(_case(geom, mode, causal), torch.float32, "pointmaps"), extra


def _module(case, **kw):
    cls = TD.CausalMUSt3R if case["causal"] else TD.MUSt3R
    dec = cls(enc_embed_dim=case["Denc"], embed_dim=case["D"], depth=case["depth"], num_heads=case["heads"], mlp_ratio=case["hidden"] / case["D"],
              feedback_type=case["feedback_type"], memory_mode=case["mode"], rope=case["rope"], eps=case["eps"], **kw)
    dec.load_state_dict(case["params"], strict=True)
    return dec.to(DEV)


def _inputs(case, c):
    B, n = case["scenes"], case["n"]
    pos = case["pos"].to(DEV).view(1, 1, n, 2).expand(B, c["V"], n, 2).contiguous()
    return pos, torch.tensor([case["H"], case["W"]]).view(1, 1, 2).expand(B, c["V"], 2).contiguous()


def _run(case, dec=None, only=None, detach=False, x_dtype=torch.float32):
    """The schedule through the module and torch.autograd: every call's x is a leaf; the loss is sum_c <pointmaps_c, G_c> (``only``: of that call alone)."""
    dec = _module(case) if dec is None else dec
    dec.zero_grad(set_to_none=True)
    xs = [c["x"].to(device=DEV, dtype=x_dtype).requires_grad_(True) for c in case["calls"]]
    mem, loss, res = None, 0, {}
    for i, (c, x) in enumerate(zip(case["calls"], xs)):
        pos, ts = _inputs(case, c)
        if detach and mem is not None:
            mem = ([m.detach() for m in mem[0]], *mem[1:])
        mem, pts, tok = dec(x, pos, ts, mem, render=c["render"], return_tokens=True)
        assert pts.shape == (case["scenes"], c["V"], case["H"], case["W"], 7) and pts.dtype == torch.float32
        res[f"tokens{i}"], res[f"pointmaps{i}"] = tok.detach().reshape(-1, case["D"]), pts.detach()
        if only is None or only == i:
            loss = loss + (pts * c["G"].to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    res.update({f"mem{l}": m.detach() for l, m in enumerate(mem[0])})
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    res.update({k: t.grad for k, t in dec.named_parameters()})
    res["tail"] = (mem[1], *mem[2:])
    return res


def _check_parity(tag, case, got, ref):
    g64, g32, extra = ref
    n = len(case["calls"])
    for i in range(n):
        p, r = got[f"pointmaps{i}"].cpu().double(), g64[f"pointmaps{i}"]
        err = float((p - r).abs().max())
        print(f"{tag} pointmaps{i}: max abs error {err:.3e} of max|out| {float(r.abs().max()):.3e}")
        assert torch.allclose(p, r, rtol=1e-5, atol=1e-4), (tag, i, err)
    names = [k for k in g64 if not k.startswith(("pointmaps", "feats"))]
    assert set(names) <= set(got)
    _compare(tag, got, {k: g64[k] for k in names}, g32, {k: v for k, v in extra.items()})
    labels, n_imgs, prot_imgs, prot_tokens = got["tail"]
    views = sum(c["V"] for c in case["calls"] if not c["render"])
    assert labels.dtype == torch.int64 and labels.shape == (case["scenes"], views * case["n"]) and n_imgs == views
    assert torch.equal(labels[0].cpu(), torch.arange(views).repeat_interleave(case["n"])) and torch.equal(labels[0], labels[-1])
    assert (prot_imgs, prot_tokens) == ((1, case["n"]) if case["causal"] else (views, views * case["n"]))


@pytest.mark.parametrize("mode", DF.DR.MODES)
@pytest.mark.parametrize("causal", [False, True], ids=["must3r", "causal"])
def test_decoder_matches_autograd_over_the_schedule(causal, mode):
    case = _case("d64", mode, causal)
    _check_parity(f"{'causal' if causal else 'must3r'} {mode}", case, _run(case), _reference("d64", mode, causal))


@pytest.mark.parametrize("geom,mode,causal", [("d128_linear", "norm_y", False), ("d128_linear", "kv", True), ("d64_nofeedback", "norm_y", False),
                                              ("d64_nofeedback", "raw", True)])
def test_decoder_other_geometries(geom, mode, causal):
    case = _case(geom, mode, causal)
    _check_parity(f"{geom} {'causal' if causal else 'must3r'} {mode}", case, _run(case), _reference(geom, mode, causal))


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) gradient routing, (e) training behaviour
# ---------------------------------------------------------------------------------------------------------------------------------
def test_gradient_reaches_the_first_call_through_the_memory_and_stops_at_a_detached_one():
    case = _case("d64", "norm_y", False)
    last = len(case["calls"]) - 1
    assert case["calls"][last]["render"]
    got = _run(case, only=last)
    for i in range(last + 1):
        assert got[f"dx{i}"] is not None and float(got[f"dx{i}"].abs().max()) > 0, i
    assert all(got[k] is not None and float(got[k].abs().max()) > 0 for k in ("feedback_layer.fc2.weight", "feedback_norm.weight", "blocks_dec.2.norm_y.weight",
                                                                             "image2_embed", "feat_embed_enc_to_dec.weight"))
    cut = _run(case, only=last, detach=True)
    assert all(cut[f"dx{i}"] is None for i in range(last)) and float(cut[f"dx{last}"].abs().max()) > 0
    assert cut["feedback_layer.fc2.weight"] is None and cut["feedback_norm.weight"] is None      # the memory that the render reads was cut from its makers
    assert float(cut["blocks_dec.0.cross_attn.projk.weight"].abs().max()) > 0
    # a memory made under no_grad is a detached one
    dec = _module(case)
    with torch.no_grad():
        mem = None
        for c in case["calls"][:last]:
            mem, _ = dec(c["x"].to(DEV), *_inputs(case, c), mem)
    assert not any(m.requires_grad for m in mem[0])
    c = case["calls"][last]
    _, pts = dec(c["x"].to(DEV), *_inputs(case, c), mem, render=True)
    assert torch.equal(pts, got[f"pointmaps{last}"])
    pts.backward(c["G"].to(DEV))
    assert torch.equal(dec.head_dec.proj.weight.grad, cut["head_dec.proj.weight"])


def test_freeze_optimizer_dtypes_and_repeats():
    case = _case("d64", "kv", True)
    dec = _module(case)
    a = _run(case, dec, x_dtype=torch.float64)
    assert all(a[f"dx{i}"].dtype == torch.float64 for i in range(len(case["calls"])))
    assert all(a[k].dtype == torch.float32 and a[k].shape == p.shape for k, p in dec.named_parameters())
    b = _run(case, dec, x_dtype=torch.float64)
    keys = [k for k in a if k != "tail"]
    assert all(torch.equal(a[k], b[k]) for k in keys), [k for k in keys if not torch.equal(a[k], b[k])]
    # an optimizer step is seen by the next forward
    opt = torch.optim.SGD(dec.parameters(), lr=1e3)
    opt.step()
    c = _run(case, dec)
    assert not torch.equal(c["tokens0"], a["tokens0"]) and not torch.equal(c[f"mem{case['depth'] - 1}"], a[f"mem{case['depth'] - 1}"])
    # frozen but the head: no gradient anywhere else
    dec = _module(case)
    dec.set_freeze("not_head")
    f = _run(case, dec)
    head = {"norm_dec.weight", "norm_dec.bias", "head_dec.proj.weight", "head_dec.proj.bias"}
    assert all((f[k] is not None) == (k in head) for k, _ in dec.named_parameters())
    assert all(torch.equal(f[k], a[k]) for k in head)
    assert all(torch.equal(f[f"pointmaps{i}"], a[f"pointmaps{i}"]) for i in range(len(case["calls"])))
