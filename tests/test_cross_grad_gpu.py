"""GPU (-m gpu): the cross-attention sublayer's and CachedDecoderBlock's training forward and backward -- csrc/train_cross.hip through
must3r_amd.train_cross -- against the yardstick tests/decblock_ref.py under CPU autograd, fed the same fp32 inputs in fp64 (truth) and in fp32 (the
reference's own precision).

Parity is the rule of tests/test_block_grad_gpu.py, unchanged: per case and tensor, ``e_gpu`` = max |GPU - fp64|, ``e_ref`` = max |fp32 CPU autograd - fp64|,
required ``e_gpu <= 4 e_ref + 32 2^-24 m`` with ``m = max|g64|``; forward outputs are held to it like gradients.  Every row is printed before it is asserted and
goes, as a table, to the file M3R_CROSS_GRAD_TABLE names (kept as profiles/cross_grad_parity.txt).  The upstream gradient is of order 1e-7.

One tensor has a magnitude of its own, the gradient of cross_attn.projk.bias where the sublayer projects every key a view sees: a shift common to a view's
keys does not move its softmax, so the true gradient is zero and max|g64| is rounding noise (update_masked on the CPU: fp64 5e-22, fp32 autograd 3.5e-13, which
is 0.89 x 2^-24 x the largest column 1-norm of the fp64 dK).  For that tensor alone ``m = max_c sum_r |dK_rc|`` of the fp64 yardstick: the magnitude of what
cancels.  (The module in the ``kv`` mode keeps the plain rule: there the memory's keys do not carry the bias.)

The exact conditions (determinism, a view / a scene alone against the batch, linearity, the segmented data gradient against the packed one, outputs that were
not asked for, canaries, pad columns, stream order) have no tolerance.
"""
import ctypes as C
import functools
import os
import time

import pytest
import torch

import decblock_ref as DR
import grad_parity as GP
from must3r_amd import _lib, train_attention as TA, train_block as TB, train_cross as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.25e11
KBIAS = "cross_attn.projk.bias"
_rows = []


def _ragged_views():
    """update_masked shifted: rows [0, 5) of x belong to no view; rows [0, 4) and [144, 149) of mem lie outside every key span"""
    out = []
    for v in TA.memory_views(2, 2, 35, 70, mask=True):
        out.append([v[0] + 5, v[1], v[2] + (4 if v[2] == 0 else 9), v[3], v[4], v[5]])
    return out


# name -> D, heads, views, M, Rm, seed, kv
CROSS = {
    "update_masked": (128, 2, TA.memory_views(2, 2, 35, 70, mask=True), 140, 280, 71, False),
    "init_pair": (128, 2, TA.memory_views(1, 2, 35, 0, mask=True), 70, 70, 72, False),
    "causal": (128, 2, TA.memory_views(1, 3, 35, 0, mask=True, causal=True), 105, 105, 73, False),
    "render": (128, 2, [[(b * 3 + j) * 17, 17, 81 * b, 81, 0, 0] for b in range(2) for j in range(3)], 102, 162, 74, False),
    "ragged": (128, 2, _ragged_views(), 145, 289, 75, False),
    "d192_kv": (192, 3, TA.memory_views(1, 2, 40, 40, mask=True), 80, 120, 76, True),
    "d768": (768, 12, TA.memory_views(1, 2, 96, 96, mask=True), 192, 288, 77, False),
}
# name -> D, heads, hidden, scenes, V, n, Nm, seed
BLOCKS = {"d128": (128, 2, 512, 2, 2, 35, 70, 81), "d768": (768, 12, 3072, 1, 2, 96, 96, 82)}

_HEADER = (
    "# tests/test_cross_grad_gpu.py: per case and tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in units of",
    "# 2^-24 m; bound = 4 e_ref + 32; ratio = e_gpu / bound.  m = max|g64|, except for cross_attn.projk.bias where every key of a view carries the",
    "# bias (true gradient zero): there m = the largest column 1-norm of the fp64 dK.  Forward outputs are held to the same bound.",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_CROSS_GRAD_TABLE"), _HEADER, _rows, (30, 28), magnitude="m")


_compare = functools.partial(GP.compare, _rows)


@functools.lru_cache(maxsize=None)
def _case(name):
    D, heads, views, M, Rm, seed, kv = CROSS[name]
    c = DR.make_cross_case(D, heads, views, M, Rm, seed, kv)
    if name == "ragged":
        c["mem"][:4] *= 1e3          # rows outside every span: large values that any stray contribution would carry into dWk / dWv
        c["mem"][144:149] *= 1e3
    return c


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(fp64 results, fp32 results, magnitudes): computed once, shared, never modified."""
    extra = {}
    g64 = DR.grads(_case(name), torch.float64, "cross", extra)
    return g64, DR.grads(_case(name), torch.float32, "cross"), ({KBIAS: extra["dK_colsum"]} if "dK_colsum" in extra else None)


@functools.lru_cache(maxsize=None)
def _block_case(geom, mode):
    D, heads, hidden, scenes, V, n, Nm, seed = BLOCKS[geom]
    return DR.make_block_case(D, heads, hidden, scenes, V, n, Nm, seed, mode=mode)


@functools.lru_cache(maxsize=None)
def _block_reference(geom, mode):
    extra = {}
    g64 = DR.grads(_block_case(geom, mode), torch.float64, "block", extra)
    return g64, DR.grads(_block_case(geom, mode), torch.float32, "block"), ({KBIAS: extra["dK_colsum"]} if mode != "kv" else None)


def _names(case):
    return ("out", "dx", "dmem") + DR.param_names(case, "cross")


def _dev(case):
    d = dict(case)
    d.update(x=case["x"].to(DEV), mem=case["mem"].to(DEV), dy=case["dy"].to(DEV), tab=torch.tensor(case["views"], dtype=torch.int32),
             params={k: v.to(DEV) for k, v in case["params"].items()})
    if "pos" in case:
        d["pos"] = case["pos"].to(DEV)
    return d


def _plist(d, kv=None):
    """the ten parameters in the order of the entry point, None for projk / projv where the memory holds k | v"""
    kv = d["mode"] == "kv" if kv is None else kv
    return [None if kv and k.split(".")[1] in ("projk", "projv") else d["params"][k] for k in DR.CROSS_PARAMS]


def _cross(d, dy=None, want=(True,) * 12, x=None, mem=None, tab=None, dmem=None, kv=None):
    """The sublayer through the direct forms: dict out, dx, dmem and the parameters' gradients (None where not asked for)."""
    p = _plist(d, kv)
    x = d["x"] if x is None else x
    mem = d["mem"] if mem is None else mem
    tab = d["tab"] if tab is None else tab
    dy = d["dy"] if dy is None else dy
    out = TC.cross_forward(x, mem, tab, *p, d["eps"])
    g = TC.cross_grad(x, mem, tab, *p, dy, d["eps"], want=want, dmem=dmem)
    torch.cuda.synchronize()
    res = dict(zip(("out", "dx", "dmem") + DR.CROSS_PARAMS, [out, *g]))
    return {k: v for k, v in res.items() if v is not None or k in _names(d)}


def _module(case):
    blk = TC.CachedDecoderBlock(case["D"], case["heads"], case["hidden"] / case["D"], case["mode"], case["rope"], case["eps"])
    blk.load_state_dict(case["params"], strict=True)
    return blk.to(DEV)


def _block(d, dy=None, blk=None, x_grad=True, mem_grad=True):
    """The block in the update form through the module and torch.autograd: x and the memory are the leaves."""
    blk = _module(d) if blk is None else blk
    blk.zero_grad(set_to_none=True)
    x = d["x"].clone().requires_grad_(x_grad)
    mem = d["mem"].clone().requires_grad_(mem_grad)
    y = TC.memory_rows(mem, blk.prepare_y(x), d["scenes"])
    out = blk(x, y, d["pos"], d["self_views"], d["views"])
    out.backward(d["dy"] if dy is None else dy)
    torch.cuda.synchronize()
    res = dict(out=out.detach(), dx=x.grad, dmem=mem.grad)
    res.update({k: t.grad for k, t in blk.named_parameters()})
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CROSS))
def test_cross_sublayer_matches_autograd(name):
    g64, g32, mags = _reference(name)
    d = _dev(_case(name))
    got = _cross(d)
    assert set(got) == set(g64) == set(_names(d))
    _compare(f"cross {name}", got, g64, g32, mags)
    if name == "ragged":
        # rows of no view: out = x + proj.bias and dx = dy, bit for bit; memory rows outside every key span: exact zeros
        assert torch.equal(got["out"][:5], d["x"][:5] + d["params"]["cross_attn.proj.bias"]) and torch.equal(got["dx"][:5], d["dy"][:5])
        assert not bool(got["dmem"][:4].any()) and not bool(got["dmem"][144:149].any()) and bool(got["dmem"][4:144].any())
        # ... and they contribute zeros to dWk / dWv: other values in those rows change no bit of any output
        mem2 = d["mem"].clone()
        mem2[:4] = 17.0
        mem2[144:149] = -3.0e4
        other = _cross(d, mem=mem2)
        for k in got:
            assert torch.equal(got[k], other[k]), k


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("geom", list(BLOCKS))
def test_decoder_block_matches_autograd(geom, mode):
    g64, g32, mags = _block_reference(geom, mode)
    got = _block(_dev(_block_case(geom, mode)))
    assert set(got) == set(g64)
    _compare(f"block {geom} {mode}", got, g64, g32, mags)


def test_pad_columns_of_a_strided_memory_survive():
    """d192_kv: mem and dmem are [120][2 D] windows with row stride 2 D + 8 inside canary-filled buffers"""
    d = _dev(_case("d192_kv"))
    D, Rm = d["D"], d["Rm"]
    full = _cross(d)
    mbuf = torch.full((Rm + 2, 2 * D + 8), CANARY, device=DEV)
    gbuf = torch.full((Rm + 2, 2 * D + 8), CANARY, device=DEV)
    mem, dmem = mbuf[1:Rm + 1, 4:2 * D + 4], gbuf[1:Rm + 1, 4:2 * D + 4]
    mem.copy_(d["mem"])
    assert mem.stride(0) == 2 * D + 8 and mem.data_ptr() % 16 == 0
    keep = mbuf.clone()
    got = _cross(d, mem=mem, dmem=dmem)
    assert got["dmem"].data_ptr() == dmem.data_ptr()
    for k in full:
        assert torch.equal(got[k], full[k]), k
    assert torch.equal(mbuf, keep)
    inside = torch.zeros(gbuf.shape, dtype=torch.bool, device=DEV)
    inside[1:Rm + 1, 4:2 * D + 4] = True
    assert bool((gbuf[~inside] == CANARY).all()), "a float outside the dmem window was written"
    # through autograd the stride of a row-strided memory is passed through as well
    leaf = mbuf.clone().requires_grad_(True)
    x = d["x"].clone().requires_grad_(True)
    p = _plist(d)
    out = TC.cross_attention_sublayer(x, leaf[1:Rm + 1, 4:2 * D + 4], d["views"], d["heads"], *p)
    out.backward(d["dy"])
    assert torch.equal(out, full["out"]) and torch.equal(x.grad, full["dx"]) and torch.equal(leaf.grad[1:Rm + 1, 4:2 * D + 4], full["dmem"])
    assert not bool(leaf.grad[0].any()) and not bool(leaf.grad[:, :4].any())


# ---------------------------------------------------------------------------------------------------------------------------------
# exact conditions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_calls_repeat_bitwise():
    d = _dev(_case("update_masked"))
    a, b = _cross(d), _cross(d)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    m = _dev(_block_case("d128", "norm_y"))
    a, b = _block(m), _block(m)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_view_alone_and_scene_alone_equal_the_batch():
    """A view's rows of out / dx (its own rows of x, its scene's memory) and a scene's rows of dmem are the same bits alone and in the two-scene batch."""
    case = _case("update_masked")
    d = _dev(case)
    full = _cross(d)
    for i, (q0, n, k0, nk, lo, hi) in enumerate(case["views"]):
        one = _cross(d, x=d["x"][q0:q0 + n].contiguous(), dy=d["dy"][q0:q0 + n].contiguous(), mem=d["mem"][k0:k0 + nk],
                     tab=torch.tensor([[0, n, 0, nk, lo, hi]], dtype=torch.int32))
        assert torch.equal(one["out"], full["out"][q0:q0 + n]) and torch.equal(one["dx"], full["dx"][q0:q0 + n]), i
    for b in range(2):
        views = [v for v in case["views"] if v[2] == 140 * b]
        q0, k0 = views[0][0], 140 * b
        tab = torch.tensor([[v[0] - q0, v[1], 0, v[3], v[4], v[5]] for v in views], dtype=torch.int32)
        one = _cross(d, x=d["x"][q0:q0 + 70].contiguous(), dy=d["dy"][q0:q0 + 70].contiguous(), mem=d["mem"][k0:k0 + 140], tab=tab)
        assert torch.equal(one["dmem"], full["dmem"][k0:k0 + 140]), b
        assert torch.equal(one["out"], full["out"][q0:q0 + 70]) and torch.equal(one["dx"], full["dx"][q0:q0 + 70]), b


def test_backward_is_linear_in_the_upstream_gradient():
    d = _dev(_case("update_masked"))
    a, b = _cross(d), _cross(d, dy=d["dy"] * 2)
    for k in a:
        if k != "out":
            assert torch.equal(a[k] * 2, b[k]), k
    m = _dev(_block_case("d128", "norm_y"))
    a, b = _block(m), _block(m, dy=m["dy"] * 2)
    for k in a:
        if k != "out":
            assert torch.equal(a[k] * 2, b[k]), k


def test_direct_calls_equal_the_module():
    """The block through autograd is the three sublayer entry points chained: the same bits.  The key rows are a leaf here (the reference's calling form)."""
    case = _block_case("d128", "norm_y")
    d = _dev(case)
    blk = _module(case)
    x, y = d["x"].clone().requires_grad_(True), torch.randn((2 * 90, 128), generator=torch.Generator().manual_seed(5)).to(DEV).requires_grad_(True)
    views = TA.memory_views(2, 2, 35, 20, mask=True)                # 90 key rows per scene
    out = blk(x, y, d["pos"], d["self_views"], views)
    out.backward(d["dy"])
    p = d["params"]
    rope_tab, tab_s, tab_m = TB.rope_table(DEV, *case["rope"]), torch.tensor(case["self_views"], dtype=torch.int32), torch.tensor(views, dtype=torch.int32)
    pa, pc = [p[k] for k in DR.ATTN_PARAMS], [p[k] for k in DR.CROSS_PARAMS]
    pm = [p[k] for k in DR.MLP_PARAMS]
    a = TB.attn_forward(d["x"], d["pos"], tab_s, rope_tab, *pa, case["eps"])
    c = TC.cross_forward(a, y.detach(), tab_m, *pc, case["eps"])
    m = TB.mlp_forward(c, *pm, case["eps"])
    assert torch.equal(m, out.detach())
    gm = TB.mlp_grad(c, *pm, d["dy"], case["eps"])
    gc = TC.cross_grad(a, y.detach(), tab_m, *pc, gm[0], case["eps"])
    ga = TB.attn_grad(d["x"], d["pos"], tab_s, rope_tab, *pa, gc[0], case["eps"])
    torch.cuda.synchronize()
    grads = {k: t.grad for k, t in blk.named_parameters()}
    assert torch.equal(ga[0], x.grad) and torch.equal(gc[1], y.grad)
    for k, g in list(zip(DR.MLP_PARAMS, gm[1:])) + list(zip(DR.CROSS_PARAMS, gc[2:])) + list(zip(DR.ATTN_PARAMS, ga[1:])):
        assert torch.equal(g, grads[k]), k
    assert grads["norm_y.weight"] is None and grads["norm_y.bias"] is None      # the norm_y mode does not touch norm_y inside the block
    # [B, N, D] without tables: one view per batch entry that attends all of its entry's y
    xb, yb = d["x"].view(4, 35, 128), y.detach().view(4, 45, 128)
    ref = blk(d["x"], y.detach(), d["pos"], TA.self_views(1, 4, 35), [[b * 35, 35, b * 45, 45, 0, 0] for b in range(4)])
    assert torch.equal(blk(xb, yb, d["pos"].view(4, 35, 2)).view(140, 128), ref)


def test_segmented_data_gradient_equals_the_packed_one():
    """dmem = dK Wk + dV Wv from the two-segment launch against must3r_hip_op_linear_dgrad_f32 on the packed dK | dV and torch.cat([Wk, Wv]), bit for bit.  The
    packed dK | dV is rebuilt by the kv-mode call on the same projected k | v."""
    d = _dev(_case("update_masked"))
    p = d["params"]
    only = tuple(n == "dmem" for n in TC.CROSS_OUTPUTS)
    dmem = _cross(d, want=only)["dmem"]
    Wk, bk, Wv, bv = (p[f"cross_attn.{n}"] for n in ("projk.weight", "projk.bias", "projv.weight", "projv.bias"))
    kv = torch.cat([TB.linear_forward(d["mem"], Wk, bk), TB.linear_forward(d["mem"], Wv, bv)], dim=1)
    dkv = _cross(d, mem=kv, want=only, kv=True)["dmem"]
    assert dkv.shape == (d["Rm"], 2 * d["D"])
    # TB.linear_grad reads W as [N, K] = [2 D, D], the packed copy of Wk over Wv, and x for its shape only
    packed = TB.linear_grad(torch.empty((d["Rm"], d["D"]), device=DEV), torch.cat([Wk, Wv]), dkv, want=(True, False, False))[0]
    torch.cuda.synchronize()
    assert torch.equal(dmem, packed)
    assert torch.equal(dmem, _cross(d)["dmem"])


ALL = TC.CROSS_OUTPUTS
WANTS = {
    "all": ALL,
    "memory_side": ("dmem", "dWk", "dbk", "dWv", "dbv"),
    "query_side": ("dx", "dgamma", "dbeta", "dWq", "dbq"),
    "dbproj_only": ("dbproj",),
    "x_only": ("dx",),
    "dmem_only": ("dmem",),
    "weights_frozen": ("dx", "dmem", "dgamma", "dbeta"),
    "norms_frozen": tuple(n for n in ALL if n not in ("dgamma", "dbeta")),
}


@pytest.mark.parametrize("want", list(WANTS))
def test_unrequested_outputs_and_canaries(want):
    """The twelve gradients lie in one canary-filled allocation with 64 canaries around each.  An output that is not asked for is NULL; its floats and every
    canary must survive, the rest is written completely and equals the full run bit for bit."""
    lib = _lib.load()
    d = _dev(_case("update_masked"))
    M, Rm, D, PAD = d["M"], d["Rm"], d["D"], 64
    full = _cross(d)
    sizes = [M * D, Rm * D, D, D, D * D, D, D * D, D, D * D, D, D * D, D]
    buf = torch.full((sum(sizes) + PAD * (len(sizes) + 1),), CANARY, device=DEV)
    off, o = [], PAD
    for s in sizes:
        off.append(o)
        o += s + PAD
    a = TC._cross_args(d["x"], d["mem"], d["tab"], *_plist(d), d["eps"])
    a.dy, a.lddmem = C.c_void_p(d["dy"].data_ptr()), D
    for f, o in zip(ALL, off):
        setattr(a, f, C.c_void_p(buf.data_ptr() + 4 * o) if f in WANTS[want] else None)
    nb = lib.must3r_hip_cross_sublayer_scratch_bytes(M, Rm, D, len(d["views"]), 0)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.must3r_hip_cross_sublayer_grad(C.byref(a), C.c_void_p(scratch.data_ptr()), nb))
    torch.cuda.synchronize()
    written = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    for f, n, o, s in zip(ALL, ("dx", "dmem") + DR.CROSS_PARAMS, off, sizes):
        if f in WANTS[want]:
            written[o:o + s] = True
            assert torch.equal(buf[o:o + s], full[n].reshape(-1)), n
    assert bool((buf[~written] == CANARY).all()), "a float outside the requested outputs was written"


@pytest.mark.parametrize("frozen", ["norms", "weights", "x", "memory"])
def test_needs_input_grad_combinations(frozen):
    d = _dev(_block_case("d128", "norm_y"))
    blk = _module(d)
    full = _block(d, blk=blk)
    for k, t in blk.named_parameters():
        if (frozen == "norms" and k.startswith("norm")) or (frozen == "weights" and not k.startswith("norm")):
            t.requires_grad_(False)
    got = _block(d, blk=blk, x_grad=frozen != "x", mem_grad=frozen != "memory")
    assert (got["dx"] is None) == (frozen == "x") and (got["dmem"] is None) == (frozen == "memory")
    for k in ("dx", "dmem"):
        if got[k] is not None:
            assert torch.equal(got[k], full[k]), k
    for k, t in blk.named_parameters():
        assert (t.grad is None) == (not t.requires_grad), k
        if t.requires_grad:
            assert t.grad.dtype == t.dtype and t.grad.shape == t.shape and torch.equal(t.grad, full[k]), k


def test_gradients_come_back_in_the_dtype_of_their_inputs():
    d = _dev(_case("init_pair"))
    x, mem = d["x"].half().requires_grad_(True), d["mem"].double().requires_grad_(True)
    out = TC.cross_attention_sublayer(x.view(2, 35, 128), mem, d["views"], 2, *_plist(d))
    out.sum().backward()
    assert out.dtype == torch.float32 and out.shape == (2, 35, 128) and x.grad.dtype == torch.float16 and x.grad.shape == x.shape
    assert mem.grad.dtype == torch.float64 and mem.grad.shape == mem.shape


def test_optimizer_step_is_seen_by_the_next_forward():
    case = _block_case("d128", "kv")
    d = _dev(case)
    blk = _module(case)
    opt = torch.optim.SGD(blk.parameters(), lr=1e4)

    def run(b):
        y = TC.memory_rows(d["mem"], b.prepare_y(d["x"]), d["scenes"])
        return b(d["x"], y, d["pos"], d["self_views"], d["views"])
    before = run(blk)
    before.backward(d["dy"])
    assert all(t.grad is not None for t in blk.parameters())
    opt.step()
    after = run(blk)
    fresh = TC.CachedDecoderBlock(case["D"], case["heads"], case["hidden"] / case["D"], "kv").to(DEV)
    fresh.load_state_dict(blk.state_dict())
    assert not torch.equal(after, before) and torch.equal(after, run(fresh))


@pytest.mark.parametrize("which", ["x", "memory", "weight"])
def test_in_place_change_of_a_saved_input_raises(which):
    d = _dev(_case("init_pair"))
    p = [t.clone().requires_grad_(True) for t in _plist(d)]
    x, mem = d["x"].clone().requires_grad_(True), d["mem"].clone().requires_grad_(True)
    xin, min_ = x * 1.0, mem * 1.0
    out = TC.cross_attention_sublayer(xin, min_, d["views"], 2, *p)
    with torch.no_grad():
        {"x": xin, "memory": min_, "weight": p[4]}[which].mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward(d["dy"])


def test_a_table_the_backward_would_refuse_is_refused_before_the_forward():
    d = _dev(_case("update_masked"))
    overlapping = [[0, 35, 0, 140, 0, 0], [35, 35, 70, 140, 0, 0]]
    x = d["x"].clone().requires_grad_(True)
    with pytest.raises(_lib.HipError, match="overlapping"):
        TC.cross_attention_sublayer(x, d["mem"], overlapping, 2, *_plist(d))
    assert TC.cross_attention_sublayer(d["x"], d["mem"], overlapping, 2, *_plist(d)).shape == d["x"].shape     # the forward alone sums nothing over views
    with pytest.raises(ValueError, match="reaches past"):
        TC.cross_attention_sublayer(d["x"], d["mem"][:100], d["views"], 2, *_plist(d))


# ---------------------------------------------------------------------------------------------------------------------------------
# stream order: the stream travels in the descriptor
# ---------------------------------------------------------------------------------------------------------------------------------
def _stream_call(bufs, d):
    """both entry points on the current stream (through _lib.stream_ptr), on the bound input buffers"""
    p = [bufs[k] for k in DR.CROSS_PARAMS]
    out = TC.cross_forward(bufs["x"], bufs["mem"], d["tab"], *p, d["eps"])
    g = TC.cross_grad(bufs["x"], bufs["mem"], d["tab"], *p, bufs["dy"], d["eps"])
    return [out, *g]


def test_both_entry_points_run_on_the_descriptors_stream():
    """The protocol of tests/test_stream_order_gpu.py: reference bits of two input sets A and B on the default stream; then, with the inputs holding B, on a side
    stream the null stream overtakes: a delay, copies of A, the calls with a->stream = the side stream, clones of the outputs, B back.  The clones must be A's
    bits and the delay must still be running when the calls have returned.  Control: the same calls with a->stream = NULL reproduce B's bits."""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay, null_stream
    delay = Delay()
    A, B = _dev(_case("update_masked")), _dev(DR.make_cross_case(128, 2, CROSS["update_masked"][2], 140, 280, 79))
    flat = lambda d: {"x": d["x"], "mem": d["mem"], "dy": d["dy"], **{k: d["params"][k] for k in DR.CROSS_PARAMS}}
    src = {"A": flat(A), "B": flat(B)}
    bufs = {k: torch.empty_like(v) for k, v in src["A"].items()}

    def load(which):
        for k, v in src[which].items():
            bufs[k].copy_(v)
    ref = {}
    for which in ("A", "A", "B"):
        load(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = _stream_call(bufs, A)
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
        outs = _stream_call(bufs, A)
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = [t.clone() for t in outs]
        load("B")
    s.synchronize()
    print(f"cross_sublayer: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
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
            outs = _stream_call(bufs, A)
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.cuda.default_stream().synchronize()
            got = [t.clone() for t in outs]
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    assert premise, f"the delay ({ms:.1f} ms) ended before the null stream was idle"
    for i, (g, r) in enumerate(zip(got, ref["B"])):
        assert torch.equal(g, r), f"output {i}: a call on the null stream did not give the decoy's bits"
