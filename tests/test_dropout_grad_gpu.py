"""GPU (-m gpu): memory dropout -- the key masks of the fp32 attention kernels (csrc/train_attention.hip, must3r_hip_attn_masked_*), through the cross sublayer
and the decoder block (must3r_hip_cross_sublayer_masked_*) up to must3r_amd.train_dropout.CausalMUSt3R -- against the yardstick tests/dropout_ref.py under
CPU autograd, fed the same fp32 inputs in fp64 (truth) and in fp32 (the reference's own precision).

Parity is the rule of tests/grad_parity.py, unchanged: ``e_gpu <= 4 e_ref + 32 2^-24 m`` per tensor; forward outputs are held to it like gradients; the
gradient of cross_attn.projk.bias has the magnitude of what cancels, as in tests/test_cross_grad_gpu.py.  Every row is printed before it is asserted and goes,
as a table, to the file M3R_DROPOUT_GRAD_TABLE names (kept as profiles/dropout_grad_parity.txt).

Kernel shape: heads 2, 2 scenes x 3 views, nq = 70, 200 key rows per scene (four key tiles, the last of 8 rows), mask_ld = 8.  The tables are the two forms of
train_attention.memory_views on those 200 rows (Nm = 20 memory rows and three 60-row slots; the kernels do not tie a view's query count to its slot): the
own-slot skip and the causal prefixes.  Mask rows: r0 random keep 0.7, r1 zero on the whole key tile [64, 128) and random elsewhere, r2 all zero, r3 all ones;
r0 and r1 are both zero on a few chosen rows; view_mask = [0, 1, 2, 3, -1, 1].  The exact properties have no tolerance.
"""
import functools
import os
import time

import pytest
import torch

import decblock_ref as DR
import dropout_ref as DO
import grad_parity as GP
from must3r_amd import _lib, train_attention as TA, train_cross as TC, train_decoder as TD, train_dropout as TDO
from test_dropout_grad_host import FIXTURE, _recorded_selections

pytestmark = pytest.mark.gpu
DEV = "cuda"
KBIAS = "cross_attn.projk.bias"
_rows = []
_HEADER = (
    "# tests/test_dropout_grad_gpu.py: per case and tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in units of",
    "# 2^-24 m; bound = 4 e_ref + 32; ratio = e_gpu / bound.  m = max|g64|, except for cross_attn.projk.bias (true gradient zero): there m = the",
    "# largest column 1-norm of the fp64 dK.  Forward outputs are held to the same bound.  Key masks in every case (memory dropout).",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_DROPOUT_GRAD_TABLE"), _HEADER, _rows, (30, 44), magnitude="m")


_compare = functools.partial(GP.compare, _rows)

# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
HEADS, SCENES, V, NQ, NK, NM, SLOT, LD = 2, 2, 3, 70, 200, 20, 60, 8
BOTH_ZERO = (5, 70, 75, 150, 199)          # rows that r0 and r1 both drop: with r2 all zero, no view of scene 0 keeps them
VIEW_MASK = [0, 1, 2, 3, -1, 1]


def _views(form):
    out = []
    for b in range(SCENES):
        for j in range(V):
            q0, k0 = (b * V + j) * NQ, b * NK
            if form == "full":
                out.append([q0, NQ, k0, NK, 0, 0])
            elif form == "skip":
                out.append([q0, NQ, k0, NK, NM + j * SLOT, NM + (j + 1) * SLOT])
            else:
                out.append([q0, NQ, k0, NM + j * SLOT, 0, 0])
    return out


@functools.lru_cache(maxsize=None)
def _kernel_case():
    g = torch.Generator().manual_seed(91)
    D = HEADS * 64
    keep = torch.zeros((4, NK), dtype=torch.bool)
    keep[0] = torch.rand(NK, generator=g) < 0.7
    keep[1] = torch.rand(NK, generator=g) < 0.7
    keep[1, 64:128] = False
    keep[3] = True
    for r in BOTH_ZERO:
        keep[0, r] = keep[1, r] = False
    return dict(q=torch.randn((SCENES * V * NQ, D), generator=g) * 2.0, k=torch.randn((SCENES * NK, D), generator=g), v=torch.randn((SCENES * NK, D), generator=g),
                dO=torch.randn((SCENES * V * NQ, D), generator=g) * 1e-7, heads=HEADS, keep=keep)


def _ref_case(form):
    c = dict(_kernel_case())
    c["views"] = _views(form)
    c["keeps"] = [None if r < 0 else c["keep"][r] for r in VIEW_MASK]
    return c


@functools.lru_cache(maxsize=None)
def _kernel_reference(form):
    return DO.attention_grads(_ref_case(form), torch.float64), DO.attention_grads(_ref_case(form), torch.float32)


def _gpu(c):
    return {k: c[k].to(DEV) for k in ("q", "k", "v", "dO")}


def _run_kernels(views, keep=None, view_mask=None, t=None, want=(True, True, True)):
    """the direct forms: dict O, lse, dQ, dK, dV"""
    t = _gpu(_kernel_case()) if t is None else t
    tab = TA._table(views)
    mask = None if keep is None else TA._mask(TA.pack_key_mask(keep.to(DEV)), view_mask, tab, torch.device(DEV, torch.cuda.current_device()))
    o, lse = TA.attention_forward(t["q"], t["k"], t["v"], tab, HEADS, want_lse=True, mask=mask)
    dq, dk, dv = TA.attention_grad(t["q"], t["k"], t["v"], t["dO"], tab, HEADS, want=want, mask=mask)
    torch.cuda.synchronize()
    return dict(O=o, lse=lse, dQ=dq, dK=dk, dV=dv)


def _same(a, b, names=("O", "lse", "dQ", "dK", "dV"), rows=None):
    for k in names:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert torch.equal(x, y), k


@pytest.mark.parametrize("form", ["skip", "causal"])
def test_masked_kernels_match_fp64(form):
    c = _kernel_case()
    assert TA.pack_key_mask(c["keep"]).shape == (4, LD)
    got = _run_kernels(_views(form), c["keep"], VIEW_MASK)
    g64, g32 = (dict(g) for g in _kernel_reference(form))
    # lse: -inf exactly where the yardstick has it (the r2 view; view 0 of the causal form keeps memory rows), the bound elsewhere
    none = torch.isinf(g64["lse"])
    assert torch.equal(torch.isinf(got["lse"]).cpu(), none) and bool((got["lse"].cpu()[none] < 0).all()) and bool(none[2 * NQ:3 * NQ].all())
    got = dict(got, lse=got["lse"].masked_fill(none.to(DEV), 0.0))
    g64["lse"], g32["lse"] = g64["lse"].masked_fill(none, 0.0), g32["lse"].masked_fill(none, 0.0)
    _compare(f"kernels {form}", got, g64, g32)
    # the r2 view: O = 0 and dQ = 0 exactly
    r2 = slice(2 * NQ, 3 * NQ)
    assert not bool(got["O"][r2].any()) and not bool(got["dQ"][r2].any())
    # key rows that every view of scene 0 drops: dK = dV = 0 exactly, and their neighbours are not
    for r in BOTH_ZERO:
        assert not bool(got["dK"][r].any()) and not bool(got["dV"][r].any()), r
    assert bool(got["dK"][:NM].any()) and bool(got["dV"][:NM].any())


@pytest.mark.parametrize("form", ["skip", "causal"])
def test_unmasked_rows_have_the_bits_of_the_unmasked_entry_points(form):
    c = _kernel_case()
    plain = _run_kernels(_views(form))
    got = _run_kernels(_views(form), c["keep"], VIEW_MASK)
    _same(got, plain, ("O", "lse", "dQ"), slice(3 * NQ, 5 * NQ))                    # views 3 (r3: all ones) and 4 (-1)
    _same(_run_kernels(_views(form), c["keep"], [3, -1, 3, -1, -1, 3]), plain)      # nothing dropped anywhere: every output
    assert not torch.equal(got["O"][:NQ], plain["O"][:NQ])


def test_a_mask_equal_to_a_skip_or_a_prefix_has_the_bits_of_the_table():
    """the tile walk and the order of additions are those of the unmasked call with the interval / prefix in its table"""
    for form in ("skip", "causal"):
        keep = torch.stack([(torch.arange(NK) < v[3]) & ~((torch.arange(NK) >= v[4]) & (torch.arange(NK) < v[5])) for v in _views(form)[:V]])
        got = _run_kernels(_views("full"), keep, [0, 1, 2] * SCENES)
        _same(got, _run_kernels(_views(form)))


def test_calls_repeat_and_a_scene_alone_has_the_batchs_bits():
    c = _kernel_case()
    a, b = _run_kernels(_views("skip"), c["keep"], VIEW_MASK), _run_kernels(_views("skip"), c["keep"], VIEW_MASK)
    _same(a, b)
    t = _gpu(c)
    alone = _run_kernels(_views("skip")[:V], c["keep"], VIEW_MASK[:V], {"q": t["q"][:V * NQ].contiguous(), "k": t["k"][:NK].contiguous(),
                                                                        "v": t["v"][:NK].contiguous(), "dO": t["dO"][:V * NQ].contiguous()})
    for k in ("O", "lse", "dQ"):
        assert torch.equal(alone[k], a[k][:V * NQ]), k
    for k in ("dK", "dV"):
        assert torch.equal(alone[k], a[k][:NK]), k


def test_autograd_operator_and_its_refusals():
    c, t = _kernel_case(), _gpu(_kernel_case())
    bits = TA.pack_key_mask(c["keep"].to(DEV))
    q, k, v = (t[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    o = TA.attention(q, k, v, _views("skip"), HEADS, key_mask=bits, view_mask=VIEW_MASK)
    o.backward(t["dO"])
    direct = _run_kernels(_views("skip"), c["keep"], VIEW_MASK)
    assert torch.equal(o, direct["O"]) and torch.equal(q.grad, direct["dQ"]) and torch.equal(k.grad, direct["dK"]) and torch.equal(v.grad, direct["dV"])
    with pytest.raises(ValueError, match="dtype=None"):
        TA.attention(q, k, v, _views("skip"), HEADS, dtype=_lib.F16, key_mask=bits, view_mask=VIEW_MASK)
    with pytest.raises(ValueError, match="come together"):
        TA.attention(q, k, v, _views("skip"), HEADS, key_mask=bits)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the cross sublayer and the block: the smallest case of tests/test_cross_grad_gpu.py (D 128, 2 scenes x 2 views of 35 over Nm = 70), three memory modes
# ---------------------------------------------------------------------------------------------------------------------------------
SUB_VIEW_MASK = [0, 1, -1, 0]


@functools.lru_cache(maxsize=None)
def _sub_keep():
    g = torch.Generator().manual_seed(92)
    keep = torch.rand((2, 140), generator=g) < 0.7
    keep[1, 64:128] = False
    keep[0, 3] = keep[1, 3] = False      # dropped by both views of scene 0; its neighbours are kept by both
    keep[:, 2] = keep[:, 4] = True
    return keep


@functools.lru_cache(maxsize=None)
def _cross_case(kv):
    return DR.make_cross_case(128, 2, TA.memory_views(2, 2, 35, 70, mask=True), 140, 280, 71, kv)


@functools.lru_cache(maxsize=None)
def _block_case(mode):
    return DR.make_block_case(128, 2, 512, 2, 2, 35, 70, 81, mode=mode)


def _sub_keeps():
    return [None if r < 0 else _sub_keep()[r] for r in SUB_VIEW_MASK]


@functools.lru_cache(maxsize=None)
def _sub_reference(which, key):
    case = _cross_case(key) if which == "cross" else _block_case(key)
    extra = {}
    g64 = DO.sublayer_grads(case, torch.float64, which, _sub_keeps(), extra)
    return g64, DO.sublayer_grads(case, torch.float32, which, _sub_keeps()), ({KBIAS: extra["dK_colsum"]} if "dK_colsum" in extra else None)


@pytest.mark.parametrize("kv", [False, True], ids=["tokens", "kv"])
def test_masked_cross_sublayer_matches_autograd(kv):
    case = _cross_case(kv)
    g64, g32, mags = _sub_reference("cross", kv)
    x, mem = case["x"].to(DEV).requires_grad_(True), case["mem"].to(DEV).requires_grad_(True)
    p = {k: case["params"][k].to(DEV).requires_grad_(True) for k in DR.param_names(case, "cross")}
    plist = [p.get(k) for k in DR.CROSS_PARAMS]
    bits = TA.pack_key_mask(_sub_keep().to(DEV))
    out = TC.cross_attention_sublayer(x, mem, case["views"], 2, *plist, case["eps"], key_mask=bits, view_mask=SUB_VIEW_MASK)
    out.backward(case["dy"].to(DEV))
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dx=x.grad, dmem=mem.grad, **{k: t.grad for k, t in p.items()})
    assert set(got) == set(g64)
    _compare(f"cross {'kv' if kv else 'tokens'}", got, g64, g32, mags)
    if kv:   # memory row 3 of scene 0 is dropped by both of its views: dK | dV = 0 exactly
        assert not bool(got["dmem"][3].any()) and bool(got["dmem"][2].any()) and bool(got["dmem"][4].any())
    # without masks the masked entry points are the unmasked ones, bit for bit
    tab = TA._table(case["views"])
    f32 = [None if t is None else t.detach() for t in plist]
    a = TC.cross_forward(x.detach(), mem.detach(), tab, *f32, case["eps"])
    none = (torch.zeros((1, 2), dtype=torch.int32, device=DEV), torch.full((4,), -1, dtype=torch.int32))
    b = TC.cross_forward(x.detach(), mem.detach(), tab, *f32, case["eps"], mask=none)
    ga = TC.cross_grad(x.detach(), mem.detach(), tab, *f32, case["dy"].to(DEV), case["eps"])
    gb = TC.cross_grad(x.detach(), mem.detach(), tab, *f32, case["dy"].to(DEV), case["eps"], mask=none)
    assert torch.equal(a, b) and all((s is None and t is None) or torch.equal(s, t) for s, t in zip(ga, gb))


@pytest.mark.parametrize("mode", DR.MODES)
def test_masked_decoder_block_matches_autograd(mode):
    case = _block_case(mode)
    g64, g32, mags = _sub_reference("block", mode)
    blk = TC.CachedDecoderBlock(case["D"], case["heads"], case["hidden"] / case["D"], mode, case["rope"], case["eps"])
    blk.load_state_dict(case["params"], strict=True)
    blk = blk.to(DEV)
    x, mem = case["x"].to(DEV).requires_grad_(True), case["mem"].to(DEV).requires_grad_(True)
    y = TC.memory_rows(mem, blk.prepare_y(x), case["scenes"])
    out = blk(x, y, case["pos"].to(DEV), case["self_views"], case["views"], key_mask=TA.pack_key_mask(_sub_keep().to(DEV)), view_mask=SUB_VIEW_MASK)
    out.backward(case["dy"].to(DEV))
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dx=x.grad, dmem=mem.grad, **{k: t.grad for k, t in blk.named_parameters()})
    assert set(got) == set(g64)
    _compare(f"block {mode}", got, g64, g32, mags if mode != "kv" else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the decoder: the fixture's case with the recorded selection injected
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _selections(dropout_mode):
    import numpy as np
    return _recorded_selections(np.load(FIXTURE), dropout_mode, len(DO.SCHEDULE))


@functools.lru_cache(maxsize=None)
def _decoder_reference(dropout_mode):
    case, extra = DO.make_case("norm_y"), {}
    g64 = DO.grads(case, torch.float64, _selections(dropout_mode), dropout_mode, "pointmaps", extra)
    return g64, DO.grads(case, torch.float32, _selections(dropout_mode), dropout_mode, "pointmaps"), extra


def _module(case, cls=TDO.CausalMUSt3R, **kw):
    dec = cls(enc_embed_dim=case["Denc"], embed_dim=case["D"], depth=case["depth"], num_heads=case["heads"], mlp_ratio=case["hidden"] / case["D"],
              feedback_type=case["feedback_type"], memory_mode=case["mode"], rope=case["rope"], eps=case["eps"], protected_imgs=DO.PROTECTED_IMGS, **kw)
    dec.load_state_dict(case["params"], strict=True)
    return dec.to(DEV)


def _inputs(case, c):
    B, n = case["scenes"], case["n"]
    pos = case["pos"].to(DEV).view(1, 1, n, 2).expand(B, c["V"], n, 2).contiguous()
    return pos, torch.tensor([case["H"], case["W"]]).view(1, 1, 2).expand(B, c["V"], 2).contiguous()


def _run(case, dec, selections=None):
    dec.zero_grad(set_to_none=True)
    xs = [c["x"].to(DEV).requires_grad_(True) for c in case["calls"]]
    mem, loss, res = None, 0, {}
    for i, (c, x) in enumerate(zip(case["calls"], xs)):
        kw = {} if selections is None else dict(selection=selections[i])
        mem, pts, tok = dec(x, *_inputs(case, c), mem, render=c["render"], return_tokens=True, **kw)
        res[f"tokens{i}"], res[f"pointmaps{i}"] = tok.detach().reshape(-1, case["D"]), pts.detach()
        loss = loss + (pts * c["G"].to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    res.update({f"mem{l}": m.detach() for l, m in enumerate(mem[0])})
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    res.update({k: t.grad for k, t in dec.named_parameters()})
    res["tail"] = (mem[1], *mem[2:])
    return res


@pytest.mark.parametrize("dropout_mode", ["temporary", "permanent"])
def test_decoder_with_the_recorded_selection_matches_autograd(dropout_mode):
    case = DO.make_case("norm_y")
    g64, g32, extra = _decoder_reference(dropout_mode)
    got = _run(case, _module(case, mem_dropout=DO.P_DROP, dropout_mode=dropout_mode), _selections(dropout_mode))
    names = [k for k in g64 if not k.startswith("feats") and k not in ("tail", "labels")]
    assert set(names) <= set(got)
    _compare(f"decoder {dropout_mode}", got, {k: g64[k] for k in names}, g32, dict(extra))
    labels, n_imgs, prot_imgs, prot_tokens = got["tail"]
    assert (n_imgs, prot_imgs, prot_tokens) == (8, 1, 35) and g64["tail"].tolist() == [8, 1, 35]
    assert labels.dtype == torch.int64 and torch.equal(labels.cpu(), g64["labels"])
    assert labels.shape[1] == (8 * 35 if dropout_mode == "temporary" else 92) == got["mem0"].shape[1]


def test_no_dropout_is_the_parent_class_bit_for_bit():
    case = DO.make_case("norm_y")
    a = _run(case, _module(case, TD.CausalMUSt3R))
    b = _run(case, _module(case, mem_dropout=0.0))
    for k in a:
        if k != "tail":
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["tail"][0], b["tail"][0]) and a["tail"][1:] == b["tail"][1:]


@pytest.mark.parametrize("dropout_mode", ["temporary", "permanent"])
def test_self_drawn_run_is_finite_repeatable_and_drops_rows(dropout_mode):
    case = DO.make_case("norm_y")
    plain = _run(case, _module(case, mem_dropout=0.0))
    runs = []
    for _ in range(2):
        g = torch.Generator(device=DEV).manual_seed(17)
        runs.append(_run(case, _module(case, mem_dropout=DO.P_DROP, dropout_mode=dropout_mode, generator=g)))
    a, b = runs
    for k in a:
        if k != "tail":
            assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all()), k
    assert torch.equal(a["tail"][0], b["tail"][0]) and a["tail"][1:] == (8, 1, 35)
    last = len(case["calls"]) - 1
    if dropout_mode == "temporary":    # the render hides rows from both views; the first call (nothing to draw) is the parent's
        assert not torch.equal(a[f"tokens{last}"], plain[f"tokens{last}"]) and torch.equal(a["tokens0"], plain["tokens0"])
        assert a["mem0"].shape == plain["mem0"].shape
    else:
        assert 35 < a["mem0"].shape[1] < plain["mem0"].shape[1] and a["tail"][0].shape[1] == a["mem0"].shape[1]
        assert bool((a["tail"][0][:, 1:] >= a["tail"][0][:, :-1]).all())
    assert not torch.equal(a["tokens1"], plain["tokens1"])


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) stream order: the protocol of tests/test_stream_order_gpu.py (see tests/test_cross_grad_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _stream_protocol(name, src, call, control=True):
    """src: {"A": tensors, "B": tensors}; call(bufs) -> outputs, on the current stream"""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay, null_stream
    delay = Delay()
    bufs = {k: torch.empty_like(v) for k, v in src["A"].items()}

    def load(which):
        for k, v in src[which].items():
            bufs[k].copy_(v)
    ref = {}
    for which in ("A", "A", "B"):
        load(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = call(bufs)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        ref[which] = [t.clone() for t in outs]
    assert sum(float((a != b).float().mean()) for a, b in zip(ref["A"], ref["B"])) / len(ref["A"]) > 0.5
    ms = min(DELAY_CAP_MS, 30.0 + 10.0 * host_ms)
    assert ms < DELAY_CAP_MS or host_ms < DELAY_CAP_MS / 10
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")
        t0 = time.perf_counter()
        outs = call(bufs)
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = [t.clone() for t in outs]
        load("B")
    s.synchronize()
    print(f"{name}: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the calls took {side_ms:.3f} ms on the host)"
    for i, (g, r) in enumerate(zip(got, ref["A"])):
        assert torch.equal(g, r), f"{name} output {i}: on a side stream the bits differ from the default-stream bits (the decoy's: {torch.equal(g, ref['B'][i])})"
    if not control:
        return
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")                         # queued behind the delay: the inputs still hold the decoy
        with null_stream():
            outs = call(bufs)
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.cuda.default_stream().synchronize()
            got = [t.clone() for t in outs]
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    assert premise, f"the delay ({ms:.1f} ms) ended before the null stream was idle"
    for i, (g, r) in enumerate(zip(got, ref["B"])):
        assert torch.equal(g, r), f"{name} output {i}: a call on the null stream did not give the decoy's bits"


def test_masked_attention_entry_points_run_on_the_descriptors_stream():
    c = _kernel_case()
    g = torch.Generator().manual_seed(93)
    A = dict(_gpu(c), bits=TA.pack_key_mask(c["keep"].to(DEV)))                                 # the packed masks are an input like the others
    B = {k: (torch.randn(v.shape, generator=g) * (1e-7 if k == "dO" else 1.0)).to(DEV) for k, v in c.items() if k in ("q", "k", "v", "dO")}
    B["bits"] = TA.pack_key_mask((torch.rand(c["keep"].shape, generator=g) < 0.5).to(DEV))
    tab = TA._table(_views("skip"))

    def call(bufs):
        mask = TA._mask(bufs["bits"], VIEW_MASK, tab, bufs["q"].device)
        o, lse = TA.attention_forward(bufs["q"], bufs["k"], bufs["v"], tab, HEADS, want_lse=True, mask=mask)
        return [o, lse, *TA.attention_grad(bufs["q"], bufs["k"], bufs["v"], bufs["dO"], tab, HEADS, mask=mask)]
    _stream_protocol("attn_masked", {"A": A, "B": B}, call)


def test_masked_cross_entry_points_run_on_the_descriptors_stream():
    a, b = _cross_case(False), DR.make_cross_case(128, 2, TA.memory_views(2, 2, 35, 70, mask=True), 140, 280, 79)
    flat = lambda d: {"x": d["x"].to(DEV), "mem": d["mem"].to(DEV), "dy": d["dy"].to(DEV), **{k: d["params"][k].to(DEV) for k in DR.CROSS_PARAMS}}
    src = {"A": flat(a), "B": flat(b)}
    src["A"]["bits"] = TA.pack_key_mask(_sub_keep().to(DEV))
    src["B"]["bits"] = TA.pack_key_mask((torch.rand((2, 140), generator=torch.Generator().manual_seed(94)) < 0.5).to(DEV))
    tab = TA._table(a["views"])

    def call(bufs):
        mask = TA._mask(bufs["bits"], SUB_VIEW_MASK, tab, bufs["x"].device)
        p = [bufs[k] for k in DR.CROSS_PARAMS]
        out = TC.cross_forward(bufs["x"], bufs["mem"], tab, *p, a["eps"], mask=mask)
        return [out, *TC.cross_grad(bufs["x"], bufs["mem"], tab, *p, bufs["dy"], a["eps"], mask=mask)]
    _stream_protocol("cross_sublayer_masked", src, call)


def test_temporary_mode_forward_issues_no_host_synchronisation():
    """The decoder's forward in the temporary mode, self-drawn, behind a delay on a side stream: it returns while the delay is still running, and its outputs
    are those of the default stream under the same seed.  Depth 2: a forward uploads two view tables per layer through the attention core's ring of four
    pinned slots, and a fifth upload behind one delay waits for the first copy (include/must3r_hip.h, "stream order") -- a property of that ring, not of
    dropout.  An update of three views over a memory and a render, so that masks are drawn, packed and applied.  The runs on the default stream come first,
    so the one host read per positions tensor (train_block.check_positions) has happened before the side stream is used."""
    import decoder_ref as DF
    case = DF.make_case(depth=2, causal=True, schedule=((2, False), (3, False), (2, True)), seed=74)
    dec = _module(case, mem_dropout=DO.P_DROP, dropout_mode="temporary")
    gen = torch.Generator(device=DEV)
    dec.mem_dropout.generator = gen
    with torch.no_grad():
        mem, _ = dec(case["calls"][0]["x"].to(DEV), *_inputs(case, case["calls"][0]))
        mem2, _ = dec(case["calls"][1]["x"].to(DEV), *_inputs(case, case["calls"][1]), mem)
    # flattened positions: the position check of train_block reads a tensor on the host once and recognises the same object afterwards
    inputs = {i: (_inputs(case, case["calls"][i])[0].reshape(-1, 2).clone(), _inputs(case, case["calls"][i])[1]) for i in (1, 2)}
    for i, m, render in ((1, mem, False), (2, mem2, True)):
        xa, xb = case["calls"][i]["x"].to(DEV), torch.randn(case["calls"][i]["x"].shape, generator=torch.Generator().manual_seed(95)).to(DEV)

        def call(bufs, i=i, m=m, render=render):
            gen.manual_seed(23)
            with torch.no_grad():
                out, pts, tok = dec(bufs["x"], *inputs[i], m, render=render, return_tokens=True)
            return [pts, tok] + ([] if render else list(out[0]))
        _stream_protocol(f"decoder temporary {'render' if render else 'update'}", {"A": {"x": xa}, "B": {"x": xb}}, call, control=False)
