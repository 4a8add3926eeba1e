"""GPU (-m gpu): the attention core's training forward and backward -- csrc/train_attention.hip ``must3r_hip_attn_forward_f32`` /
``must3r_hip_attn_grad`` through must3r_amd.train_attention -- against the yardstick tests/attn_grad_ref.py under CPU autograd, fed the same fp32
inputs in fp64 (truth) and in fp32 (the reference's own precision).

Parity is the rule of tests/test_loss_grad_gpu.py and tests/test_head_grad_gpu.py, unchanged: per case and tensor, ``e_gpu`` = max |GPU - fp64|,
``e_ref`` = max |fp32 CPU autograd - fp64|, required ``e_gpu <= 4 e_ref + 32 2^-24 max|g64|``; the fp32 forward's O is held to it like a gradient.
Every row is printed before it is asserted and goes, as a table, to the file M3R_ATTN_GRAD_TABLE names (kept as profiles/attn_grad_parity.txt).  The
upstream gradient is of order 1e-7, below fp16's range.

The exact conditions (determinism, independence of a view's dQ and of a scene's dK / dV from the rest of the batch, linearity, zero upstream
gradients, outputs that were not asked for, canaries, the F16 forward's bits) have no tolerance.
"""
import ctypes as C
import functools
import os

import pytest
import torch

import attn_grad_ref as AR
import grad_parity as GP
from must3r_amd import _lib, train_attention as TA

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.25e11
_rows = []

_HEADER = (
    "# tests/test_attn_grad_gpu.py: per case and tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in units of",
    "# 2^-24 max|g64|; bound = 4 e_ref + 32; ratio = e_gpu / bound.  O is the fp32 forward's output, held to the same bound.",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_ATTN_GRAD_TABLE"), _HEADER, _rows, (34, 10), worst=False)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(case, fp64 results, fp32 results): computed once, shared, never modified."""
    case = AR.make_case(name)
    return case, AR.grads(case, torch.float64), AR.grads(case, torch.float32)


def _dev(case):
    """The case on the GPU; a packed case keeps q, k, v as column slices of the packed tensor."""
    d = dict(case)
    if case["qkv"] is not None:
        D = case["heads"] * 64
        qkv = case["qkv"].to(DEV)
        d.update(qkv=qkv, q=qkv[:, :D], k=qkv[:, D:2 * D], v=qkv[:, 2 * D:])
    else:
        d.update({n: case[n].to(DEV) for n in ("q", "k", "v")})
    d["dO"] = case["dO"].to(DEV)
    d["tab"] = torch.tensor(case["views"], dtype=torch.int32)
    return d


def _gpu(d, dO=None, want=(True, True, True), views=None):
    tab = d["tab"] if views is None else torch.tensor(views, dtype=torch.int32)
    o = TA.attention_forward(d["q"], d["k"], d["v"], tab, d["heads"])
    dq, dk, dv = TA.attention_grad(d["q"], d["k"], d["v"], d["dO"] if dO is None else dO, tab, d["heads"], want=want)
    torch.cuda.synchronize()
    return dict(O=o, dQ=dq, dK=dk, dV=dv)


_compare = functools.partial(GP.compare, _rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AR.CASES)
def test_forward_and_gradients_match_autograd(name):
    """self_ragged: a full 64-tile and a 6-row tail on both axes, packed operands (leading dimensions, head indexing); self_tiny: all tail;
    self_12h: full tiles, 12 heads, a peaked softmax; cross_shared: three views per scene share their key rows, skips that start and end on and inside
    tiles; cross_whole_tile: a skip that contains a whole key tile; causal: nested prefixes in one group, the excluded [0, n) form; degenerate: a
    view without keys and one whose skip covers all of them beside a normal view."""
    case, g64, g32 = _reference(name)
    got = _gpu(_dev(case))
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    _compare(name, got, g64, g32)


def test_degenerate_views_are_exact():
    case, _, _ = _reference("degenerate")
    d = _dev(case)
    got, alone = _gpu(d), _gpu(d, views=case["views"][:1])
    assert bool((got["O"][40:] == 0).all()) and bool((got["dQ"][40:] == 0).all())
    assert torch.equal(got["dK"], alone["dK"]) and torch.equal(got["dV"], alone["dV"]) and float(got["dK"].abs().max()) > 0
    assert torch.equal(got["O"][:40], alone["O"][:40]) and torch.equal(got["dQ"][:40], alone["dQ"][:40])
    o, lse = TA.attention_forward(d["q"], d["k"], d["v"], d["tab"], d["heads"], want_lse=True)
    assert bool(torch.isfinite(lse[:40]).all()) and bool((lse[40:] == float("-inf")).all())


def test_lse_is_the_log_of_the_row_sum():
    case, _, _ = _reference("cross_shared")
    d = _dev(case)
    _, lse = TA.attention_forward(d["q"], d["k"], d["v"], d["tab"], d["heads"], want_lse=True)
    ref = torch.empty(lse.shape, dtype=torch.float64)
    q, k = case["q"].double(), case["k"].double()
    for view in case["views"]:
        q0, nq, k0, nk, _, _ = view
        for h in range(case["heads"]):
            s = q[q0:q0 + nq, h * 64:(h + 1) * 64] @ k[k0:k0 + nk, h * 64:(h + 1) * 64].t() / 8
            ref[q0:q0 + nq, h] = torch.logsumexp(s.masked_fill(~AR.valid_mask(view), float("-inf")), dim=1)
    assert torch.allclose(lse.cpu().double(), ref, rtol=0, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact conditions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["self_ragged", "cross_whole_tile"])
def test_calls_repeat_bitwise(name):
    d = _dev(_reference(name)[0])
    a, b = _gpu(d), _gpu(d)
    for k in AR.NAMES:
        assert torch.equal(a[k], b[k]), k


def test_view_alone_equals_view_in_batch():
    """dQ and O of a view do not depend on the other views of the call (self attention: nor do its dK and dV)."""
    case = _reference("self_ragged")[0]
    d = _dev(case)
    full = _gpu(d)
    for i, view in enumerate(case["views"]):
        one = _gpu(d, views=[view])
        rows = slice(view[0], view[0] + view[1])
        for k in AR.NAMES:
            assert torch.equal(one[k][rows], full[k][rows]), (i, k)
    case = _reference("cross_shared")[0]
    d = _dev(case)
    full = _gpu(d, want=(True, False, False))
    for i, view in enumerate(case["views"]):
        one = _gpu(d, views=[view], want=(True, False, False))
        rows = slice(view[0], view[0] + view[1])
        assert torch.equal(one["dQ"][rows], full["dQ"][rows]) and torch.equal(one["O"][rows], full["O"][rows]), i


@pytest.mark.parametrize("name", ["cross_shared", "causal"])
def test_scene_alone_equals_scene_beside_another(name):
    case = _reference(name)[0]
    d = _dev(case)
    full = _gpu(d)
    rk = case["k"].shape[0] // 2
    for b in range(2):
        one = _gpu(d, views=case["views"][3 * b:3 * b + 3])
        rows = slice(b * rk, (b + 1) * rk)
        other = slice((1 - b) * rk, (2 - b) * rk)
        assert torch.equal(one["dK"][rows], full["dK"][rows]) and torch.equal(one["dV"][rows], full["dV"][rows]), b
        assert bool((one["dK"][other] == 0).all()) and bool((one["dV"][other] == 0).all()), b       # rows of no group: the wrapper's zeros


def test_backward_is_linear_in_the_upstream_gradient():
    d = _dev(_reference("cross_shared")[0])
    a, b, z = _gpu(d), _gpu(d, dO=d["dO"] * 4), _gpu(d, dO=torch.zeros_like(d["dO"]))
    for k in ("dQ", "dK", "dV"):
        assert torch.equal(a[k] * 4, b[k]), k
        assert bool((z[k] == 0).all()), k


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (False, True, True), (True, True, True)], ids=str)
def test_unrequested_outputs_and_canaries(want):
    """The three gradients lie in one canary-filled allocation with 64 canaries around them, and the table leaves rows out: query rows [0, 5) and
    [75, 80) belong to no view, key rows [0, 3) and [73, 80) to no group (and rows [53, 73) only to the wider view's span).  An output that is not
    asked for is NULL; its floats, every canary and every row outside the views / groups must survive, the rest is written completely."""
    lib = _lib.load()
    heads, D, Rq, Rk, PAD = 2, 128, 80, 80, 64
    views = [[5, 40, 3, 70, 10, 20], [45, 30, 3, 50, 0, 0]]
    g = torch.Generator().manual_seed(21)
    q, k, v = (torch.randn((R, D), generator=g).to(DEV) for R in (Rq, Rk, Rk))
    dO = (torch.randn((Rq, D), generator=g) * 1e-7).to(DEV)
    tab = torch.tensor(views, dtype=torch.int32)
    sizes = dict(dQ=Rq * D, dK=Rk * D, dV=Rk * D)
    buf = torch.full((sum(sizes.values()) + PAD * 4,), CANARY, device=DEV)
    off, o = {}, PAD
    for n in sizes:
        off[n] = o
        o += sizes[n] + PAD
    a = TA._args(q, k, v, tab, heads)
    a.dO, a.lddo, a.lddq, a.lddk, a.lddv = C.c_void_p(dO.data_ptr()), D, D, D, D
    for n, w in zip(sizes, want):
        setattr(a, n, C.c_void_p(buf.data_ptr() + 4 * off[n]) if w else None)
    scratch, nb = TA._scratch(tab, heads, q.device)
    _lib.check(lib.must3r_hip_attn_grad(C.byref(a), C.c_void_p(scratch.data_ptr()), nb, C.c_void_p(_lib.stream_ptr(torch.device(DEV)))))
    torch.cuda.synchronize()
    written = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    span = dict(dQ=(5, 75), dK=(3, 73), dV=(3, 73))
    for n, w in zip(sizes, want):
        if w:
            written[off[n] + span[n][0] * D:off[n] + span[n][1] * D] = True
    assert bool((buf[~written] == CANARY).all()), "a float outside the requested outputs' rows was written"
    assert bool((buf[written] != CANARY).all()) and bool(torch.isfinite(buf[written]).all()), "a requested output was not written completely"
    full = TA.attention_grad(q, k, v, dO, tab, heads)
    for n, w, f in zip(sizes, want, full):
        if w:
            lo, hi = span[n]
            assert torch.equal(buf[off[n]:off[n] + sizes[n]].view(-1, D)[lo:hi], f[lo:hi]), n
            assert bool((f[:lo] == 0).all()) and bool((f[hi:] == 0).all()), n


def test_forward_leaves_rows_of_no_view_alone():
    lib = _lib.load()
    heads, D = 2, 128
    views = [[5, 40, 0, 70, 10, 20]]
    g = torch.Generator().manual_seed(22)
    q, k, v = (torch.randn((R, D), generator=g).to(DEV) for R in (50, 70, 70))
    tab = torch.tensor(views, dtype=torch.int32)
    o, lse = torch.full((50, D), CANARY, device=DEV), torch.full((50, heads), CANARY, device=DEV)
    a = TA._args(q, k, v, tab, heads)
    a.O, a.ldo, a.lse = C.c_void_p(o.data_ptr()), D, C.c_void_p(lse.data_ptr())
    scratch, nb = TA._scratch(tab, heads, q.device)
    _lib.check(lib.must3r_hip_attn_forward_f32(C.byref(a), C.c_void_p(scratch.data_ptr()), nb, C.c_void_p(_lib.stream_ptr(torch.device(DEV)))))
    torch.cuda.synchronize()
    for t in (o, lse):
        assert bool((t[:5] == CANARY).all()) and bool((t[45:] == CANARY).all()) and bool((t[5:45] != CANARY).all())
    assert torch.equal(o[5:45], TA.attention_forward(q, k, v, tab, heads)[5:45])


# ---------------------------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def test_autograd_end_to_end_packed_qkv():
    """loss = sum(O * dO) through ``attention`` on the three column blocks of one packed leaf: qkv.grad holds dQ | dK | dV."""
    case, g64, g32 = _reference("self_ragged")
    D = case["heads"] * 64
    qkv = case["qkv"].to(DEV).requires_grad_(True)
    o = TA.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], case["views"], case["heads"])
    assert o.dtype == torch.float32 and o.shape == (210, D)
    (o * case["dO"].to(DEV)).sum().backward()
    g = qkv.grad
    _compare("autograd self_ragged", dict(O=o, dQ=g[:, :D], dK=g[:, D:2 * D], dV=g[:, 2 * D:]), g64, g32)
    direct = _gpu(_dev(case))
    assert torch.equal(direct["dQ"], g[:, :D]) and torch.equal(direct["dK"], g[:, D:2 * D]) and torch.equal(direct["dV"], g[:, 2 * D:])


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, False), (False, False, True), (True, False, True)], ids=str)
def test_needs_input_grad_subsets(needs):
    case, _, _ = _reference("cross_shared")
    d = _dev(case)
    leaves = [d[n].clone().requires_grad_(r) for n, r in zip(("q", "k", "v"), needs)]
    o = TA.attention(*leaves, case["views"], case["heads"])
    (o * d["dO"]).sum().backward()
    full = _gpu(d)
    for t, r, n in zip(leaves, needs, ("dQ", "dK", "dV")):
        assert (t.grad is not None) == r, n
        if r:
            assert t.grad.dtype == t.dtype and t.grad.shape == t.shape and torch.equal(t.grad, full[n]), n
    # the Function itself hands back None for the rest
    ctx_out = TA._Attention.apply(*leaves, d["tab"], case["heads"], None)
    grads = torch.autograd.grad((ctx_out * d["dO"]).sum(), [t for t in leaves if t.requires_grad])
    assert len(grads) == sum(needs)


def test_f16_forward_is_the_inference_kernel_and_backward_is_fp32():
    lib = _lib.load()
    case, g64, g32 = _reference("cross_shared")
    d = _dev(case)
    heads, D = case["heads"], case["heads"] * 64
    leaves = [d[n].clone().requires_grad_(True) for n in ("q", "k", "v")]
    o = TA.attention(*leaves, case["views"], heads, dtype=_lib.F16)
    # the inference entry point on the same cast operands
    q16, k16, v16 = (d[n].half().contiguous() for n in ("q", "k", "v"))
    o16 = torch.empty((q16.shape[0], D), dtype=torch.float16, device=DEV)
    tab_dev = d["tab"].to(DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.must3r_hip_op_attention(_lib.F16, P(q16), P(k16), P(v16), P(o16), D, D, D, D, heads, P(tab_dev), len(case["views"]), 48, 0, None, 0,
                                           C.c_void_p(_lib.stream_ptr(torch.device(DEV)))))
    torch.cuda.synchronize()
    assert o.dtype == torch.float32 and torch.equal(o.detach(), o16.float())
    assert float((o.detach().cpu().double() - g64["O"]).abs().max()) < 2e-2 * float(g64["O"].abs().max())
    (o * d["dO"]).sum().backward()
    full = _gpu(d)
    for t, n in zip(leaves, ("dQ", "dK", "dV")):
        assert torch.equal(t.grad, full[n]), n
    ob = TA.attention(d["q"], d["k"], d["v"], case["views"], heads, dtype=_lib.BF16)
    assert float((ob.cpu().double() - g64["O"]).abs().max()) < 8e-2 * float(g64["O"].abs().max())


def test_overlapping_groups_are_refused_before_the_forward():
    d = _dev(_reference("self_tiny")[0])
    q = d["q"].clone().requires_grad_(True)
    big = torch.randn((12, 128), device=DEV)
    with pytest.raises(_lib.HipError, match="overlapping"):
        TA.attention(torch.randn((12, 128), device=DEV, requires_grad=True), big, big, [[0, 6, 0, 6, 0, 0], [6, 6, 3, 6, 0, 0]], 2)
    # without a gradient the same table is a plain forward
    o = TA.attention(big, big, big, [[0, 6, 0, 6, 0, 0], [6, 6, 3, 6, 0, 0]], 2)
    assert bool(torch.isfinite(o).all())
    with pytest.raises(ValueError, match="reaches past"):
        TA.attention(q, d["k"], d["v"], [[0, 7, 0, 6, 0, 0]], 2)
