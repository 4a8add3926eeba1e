"""GPU (-m gpu): the bf16 training attention core (csrc/train_attn16.hip) and the switch that selects it (``must3r_hip_train_attention_mode`` through
``train_block.attention_precision`` and ``train_block.amp``).

Exact operand checks.  A view with ONE valid key has P = 1, so the products collapse: O is that key's ``v.bfloat16().float()`` bit for bit, lse is
``s sum q^ k^`` within (64 + 8) 2^-24 s sum |q^| |k^| (63 additions, the two constant multiplications and their constants' roundings, headroom), and dV of the
key is ``sum dO^`` over the rows that read it within (n_rows + 4) 2^-24 sum |dO^|.  The single key is made in four ways (nk = 1; nk = 70 with the skip
[1, 70) and with [0, 69); a mask row of nk = 130 with bit 129 alone), for 1, 17 and 70 queries and 2 heads.  The fp32 kernels fail all three (O = v unrounded).

Parity is the rule of tests/grad_parity.py, unchanged: ``e_gpu <= 4 e_ref + 32 2^-24 m`` against the UNROUNDED fp64 yardstick.  For the core (the seven cases
of tests/attn_grad_ref.py) ``e_ref`` is the fp32 CPU run of tests/attn16_ref.py; for the attention and cross sublayers, ``CachedDecoderBlock`` in its three
memory modes and the decoder over the schedule of tests/decoder_ref.py it is fp32 CPU autograd under ``torch.autocast("cpu", bfloat16)``, as in
tests/test_linear16_gpu.py.  Every row is printed before it is asserted and goes to the file M3R_ATTN16_TABLE names (kept as profiles/attn16_parity.txt).

That rule measures the size of the bf16 rounding error (e_ref is about 10^5 units of 2^-24 m), so a wrong rounding point passes it.  The core is therefore
also held to the fp64 run of ITS OWN rounded arithmetic (``attn16_ref.core(float64, tiled=True)``) by ``grad_parity.compare_rounded``: the 0.9 quantile over
the (row, head) segments of max |GPU - y64| within ``4 q(e_ref) + 32 2^-24 m``, ``e_ref`` from the fp32 CPU run of the same arithmetic -- what is left is the
fp32 accumulation, a few units, and a whole bf16 ulp in the few segments where a p or a dS rounds to its other neighbour in fp32, which the quantile steps
over (at most a tenth of the segments; the GPU's share is printed and asserted).  lse is held entry by entry, without a quantile.  The seven cases and the
key-mask case, so both instances of all three kernels.  tests/test_attn16_host.py shows what this rule sees: all nine planted defects, in every case.

The exact conditions (repeatability, a view and a scene alone, an all-ones mask, degenerate rows, canaries, the fp32 mode untouched by the switch, a backward
in the mode of its forward, the caller's stream) have no tolerance.
"""
import ctypes as C
import functools
import os
import threading

import pytest
import torch

import attn16_ref as R16
import attn_grad_ref as AR
import block_ref as BR
import decblock_ref as DR
import decoder_ref as DF
import dropout_ref as DO
import grad_parity as GP
from must3r_amd import _lib, train_attention as TA, train_block as TB, train_cross as TC, train_decoder as TD

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
CANARY = -7.25e11
KBIAS = "cross_attn.projk.bias"
_rows = []
_rounded_rows = []
_worst = {}

_HEADER = (
    "# tests/test_attn16_gpu.py, bf16 mode of the training attention core.  e_gpu = max |GPU - fp64| against the UNROUNDED fp64 yardstick, e_ref = max |reference",
    "# run - fp64|, both in units of 2^-24 m; bound = 4 e_ref + 32; ratio = e_gpu / bound.  Core rows (the seven cases of attn_grad_ref): the reference run is the",
    "# fp32 CPU run of tests/attn16_ref.py (the kernels' arithmetic with its five roundings).  Sublayer, block and decoder rows: the reference run is fp32 CPU",
    "# autograd under torch.autocast('cpu', bfloat16); 'attn only' = attention_precision('bf16') alone, 'amp' = amp('bf16').  m = max|g64|, except for",
    "# cross_attn.projk.bias (true gradient zero): the largest column 1-norm of the fp64 dK.  Decoder rows: the worst tensor of each group.",
)
_ROUNDED_HEADER = (
    "#",
    "# rounded: the core against the fp64 run of ITS OWN rounded arithmetic (attn16_ref.core(float64, tiled=True)), grad_parity.compare_rounded.  O, dQ, dK, dV:",
    "# q e_gpu and q e_ref are the 0.9 quantile over the (row, head) segments of written rows of max |GPU - y64| and max |fp32 CPU run - y64|, in units of",
    "# 2^-24 m; bound = 4 q e_ref + 32; ratio = q e_gpu / bound; share = the share of the GPU's segments above the bound (the rule steps over 0.1).  lse: every",
    "# finite entry, no quantile: the columns are max |. - lse64| in units of 2^-24 max(1, max|lse64|), share = the share of entries above the bound.",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    lib = _lib.load()
    lib.must3r_hip_train_attention_mode(0)
    lib.must3r_hip_train_linear_mode(0)
    yield
    rows = _rows + list(_worst.values())
    GP.write_table(os.environ.get("M3R_ATTN16_TABLE"), _HEADER, rows, (34, 60), magnitude="m")
    GP.append_rounded_table(os.environ.get("M3R_ATTN16_TABLE"), _ROUNDED_HEADER, _rounded_rows, (34, 60), mode="a" if rows else "w")


@pytest.fixture(autouse=True)
def _default_mode():
    yield
    assert (TB.current_precision(), TB.current_attention_precision()) == ("fp32", "fp32"), "a test left a mode set"


bf16 = functools.partial(TB.attention_precision, "bf16")
_compare = functools.partial(GP.compare, _rows)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(case, unrounded fp64 autograd, fp32 run of the bf16 arithmetic): computed once, shared, never modified."""
    case = AR.make_case(name)
    return case, AR.grads(case, torch.float64), R16.core(case, torch.float32)


def _dev(case):
    d = dict(case)
    if case.get("qkv") is not None:
        D = case["heads"] * 64
        qkv = case["qkv"].to(DEV)
        d.update(qkv=qkv, q=qkv[:, :D], k=qkv[:, D:2 * D], v=qkv[:, 2 * D:])
    else:
        d.update({n: case[n].to(DEV) for n in ("q", "k", "v")})
    d["dO"] = case["dO"].to(DEV)
    d["tab"] = torch.tensor(case["views"], dtype=torch.int32)
    return d


def _gpu(d, dO=None, want=(True, True, True), views=None, mask=None, mode="bf16"):
    """O, lse and the gradients through the direct forms, in the named mode of the attention core"""
    tab = d["tab"] if views is None else torch.tensor(views, dtype=torch.int32)
    with TB.attention_precision(mode):
        o, lse = TA.attention_forward(d["q"], d["k"], d["v"], tab, d["heads"], want_lse=True, mask=mask)
        dq, dk, dv = TA.attention_grad(d["q"], d["k"], d["v"], d["dO"] if dO is None else dO, tab, d["heads"], want=want, mask=mask)
    torch.cuda.synchronize()
    return dict(O=o, lse=lse, dQ=dq, dK=dk, dV=dv)


def _same(a, b, keys=AR.NAMES + ("lse",)):
    return [k for k in keys if a[k] is not None and not torch.equal(a[k], b[k])]


# ---------------------------------------------------------------------------------------------------------------------------------
# exact operand checks: one valid key
# ---------------------------------------------------------------------------------------------------------------------------------
def _single_key(form, nq):
    """(views, nk, index of the valid key, keep row or None)"""
    if form == "nk1":
        return [[0, nq, 0, 1, 0, 0]], 1, 0, None
    if form == "skip_tail":
        return [[0, nq, 0, 70, 1, 70]], 70, 0, None
    if form == "skip_head":
        return [[0, nq, 0, 70, 0, 69]], 70, 69, None
    keep = torch.zeros((1, 130), dtype=torch.bool)
    keep[0, 129] = True
    return [[0, nq, 0, 130, 0, 0]], 130, 129, keep


@pytest.mark.parametrize("nq", [1, 17, 70])
@pytest.mark.parametrize("form", ["nk1", "skip_tail", "skip_head", "mask"])
def test_one_valid_key_gives_the_rounded_operands_exactly(form, nq):
    heads, D = 2, 128
    views, nk, j, keep = _single_key(form, nq)
    g = torch.Generator().manual_seed(100 + nq)
    q, k, v, dO = (torch.randn((r, D), generator=g) for r in (nq, nk, nk, nq))
    d = dict(q=q.to(DEV), k=k.to(DEV), v=v.to(DEV), dO=dO.to(DEV), heads=heads, tab=torch.tensor(views, dtype=torch.int32))
    mask = None if keep is None else TA._mask(TA.pack_key_mask(keep.to(DEV)), [0], d["tab"], torch.device(DEV, 0))
    got = {n: t.cpu() for n, t in _gpu(d, mask=mask).items()}
    # O: the key's v rounded to bf16, in every query row, bit for bit
    assert torch.equal(got["O"], v[j].bfloat16().float().expand(nq, D)), "O is not v^ of the valid key"
    # lse = s q^ . k^
    for h in range(heads):
        ref, bound = R16.lse_bound(q[:, h * 64:(h + 1) * 64], k[j, h * 64:(h + 1) * 64])
        err = (got["lse"][:, h].double() - ref).abs()
        print(f"{form} nq {nq} head {h}: worst |lse - s q^.k^| / bound {float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), (form, nq, h, float((err / bound).max()))
    # dV of the key: the column sums of dO^; every other key row: exact zeros
    do64 = dO.bfloat16().double()
    err, bound = (got["dV"][j].double() - do64.sum(0)).abs(), (nq + 4) * U * do64.abs().sum(0)
    print(f"{form} nq {nq}: worst |dV - sum dO^| / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), (form, nq, float((err / bound).max()))
    rest = torch.ones(nk, dtype=torch.bool)
    rest[j] = False
    assert not bool(got["dV"][rest].any()) and not bool(got["dK"][rest].any())


# ---------------------------------------------------------------------------------------------------------------------------------
# parity: the core
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AR.CASES)
def test_core_matches_fp64_like_its_fp32_emulation(name):
    case, g64, g32 = _reference(name)
    got = _gpu(_dev(case))
    assert all(bool(torch.isfinite(got[k]).all()) for k in AR.NAMES)
    _compare(f"core {name}", {k: got[k] for k in AR.NAMES}, g64, {k: g32[k] for k in AR.NAMES})
    fin = torch.isfinite(g32["lse"])
    assert bool(((got["lse"].cpu() == float("-inf")) == ~fin).all())
    assert torch.allclose(got["lse"].cpu()[fin], g32["lse"][fin], rtol=0, atol=1e-4)


ROUNDED_CASES = AR.CASES + ("cross_shared key mask",)


@functools.lru_cache(maxsize=None)
def _rounded_reference(name):
    """(case, keep [views, nk] or None, fp64 and fp32 runs of the rounded arithmetic in the kernel's tile order, counted rows): computed once, shared, never
    modified."""
    case, keep = R16.key_mask_case() if name == "cross_shared key mask" else (_reference(name)[0], None)
    keeps = None if keep is None else list(keep)
    return case, keep, R16.core(case, torch.float64, tiled=True, keep=keeps), R16.core(case, torch.float32, tiled=True, keep=keeps), R16.written_rows(case, keeps)


@pytest.mark.parametrize("name", ROUNDED_CASES)
def test_core_matches_the_fp64_run_of_its_own_rounding(name):
    """What is left between the GPU and the fp64 run of the same five roundings is the fp32 accumulation, and a whole bf16 ulp wherever a p or a dS rounds to
    the other neighbour in fp32: the quantile rule of ``grad_parity.compare_rounded`` on O, dQ, dK, dV, and every finite entry of lse, which no such flip
    reaches.  The key-mask case puts the MASK instances of the three kernels under the same rule."""
    case, keep, y64, r32, counted = _rounded_reference(name)
    d = _dev(case)
    mask = None if keep is None else TA._mask(TA.pack_key_mask(keep.to(DEV)), list(range(len(case["views"]))), d["tab"], d["q"].device)
    got = {k: t.cpu() for k, t in _gpu(d, mask=mask).items()}
    tag = f"rounded {name}"
    fin, bound = R16.lse_rounded_bound(y64["lse"], r32["lse"])
    unit = U * max(1.0, float(y64["lse"][fin].abs().max()))
    err = (got["lse"][fin].double() - y64["lse"][fin]).abs()
    e_gpu, e_ref = float(err.max()), float((r32["lse"][fin].double() - y64["lse"][fin]).abs().max())
    share = float((err > bound).double().mean())
    print(f"{tag} lse: e_gpu {e_gpu / unit:.2f} e_ref {e_ref / unit:.2f} (units of 2^-24 max(1, max|lse64|)) e_gpu / bound {e_gpu / bound:.3f}")
    _rounded_rows.append((tag, "lse", unit / U, e_gpu / unit, e_ref / unit, e_gpu / bound, share))
    GP.compare_rounded(_rounded_rows, tag, {k: got[k] for k in AR.NAMES}, {k: y64[k] for k in AR.NAMES}, r32, case["heads"], counted=counted)
    assert all(r[6] <= 0.1 for r in _rounded_rows if r[0] == tag), [r for r in _rounded_rows if r[0] == tag]
    assert bool(((got["lse"] == float("-inf")) == ~fin).all())
    assert e_gpu <= bound, (tag, "lse", e_gpu, e_ref, bound)


def test_bf16_output_differs_from_fp32_output():
    d = _dev(_reference("self_12h")[0])
    a, b = _gpu(d), _gpu(d, mode="fp32")
    assert _same(a, b, AR.NAMES) == list(AR.NAMES)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact conditions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["self_ragged", "cross_whole_tile"])
def test_calls_repeat_bitwise(name):
    d = _dev(_reference(name)[0])
    assert not _same(_gpu(d), _gpu(d))


def test_view_alone_equals_view_in_batch():
    case = _reference("self_ragged")[0]
    d = _dev(case)
    full = _gpu(d)
    for i, view in enumerate(case["views"]):
        one = _gpu(d, views=[view])
        rows = slice(view[0], view[0] + view[1])
        for k in AR.NAMES + ("lse",):
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
        rows, other = slice(b * rk, (b + 1) * rk), slice((1 - b) * rk, (2 - b) * rk)
        assert torch.equal(one["dK"][rows], full["dK"][rows]) and torch.equal(one["dV"][rows], full["dV"][rows]), b
        assert not bool(one["dK"][other].any()) and not bool(one["dV"][other].any()), b


def test_all_ones_mask_equals_the_unmasked_call():
    case = _reference("cross_shared")[0]
    d = _dev(case)
    keep = torch.ones((1, 224), dtype=torch.bool, device=DEV)
    mask = TA._mask(TA.pack_key_mask(keep), [0] * len(case["views"]), d["tab"], d["q"].device)
    assert not _same(_gpu(d, mask=mask), _gpu(d))


def test_masked_core_matches_the_reference_with_the_same_keys():
    """cross_shared with a random key mask per view on top of its skips: the MASK instantiations against the reference with the same keep rows."""
    case, _, _ = _reference("cross_shared")
    d = _dev(case)
    keep = torch.rand((len(case["views"]), 224), generator=torch.Generator().manual_seed(5)) < 0.6
    keep[:, 0] = True
    keep[1, 64:128] = False          # a key tile without a bit
    rows = list(range(len(case["views"])))
    mask = TA._mask(TA.pack_key_mask(keep.to(DEV)), rows, d["tab"], d["q"].device)
    got = _gpu(d, mask=mask)
    keeps = [keep[r] for r in rows]
    q, k, v = (case[n].double().clone().requires_grad_(True) for n in ("q", "k", "v"))
    o = DO.attention(q, k, v, case["views"], case["heads"], keeps)
    o.backward(case["dO"].double())
    g64 = dict(O=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)
    g32 = R16.core(case, torch.float32, keep=keeps)
    _compare("core cross_shared key mask", {n: got[n] for n in AR.NAMES}, g64, {n: g32[n] for n in AR.NAMES})


def test_degenerate_views_are_exact():
    case, _, _ = _reference("degenerate")
    d = _dev(case)
    got, alone = _gpu(d), _gpu(d, views=case["views"][:1])
    assert not bool(got["O"][40:].any()) and not bool(got["dQ"][40:].any())
    assert torch.equal(got["dK"], alone["dK"]) and torch.equal(got["dV"], alone["dV"]) and float(got["dK"].abs().max()) > 0
    assert torch.equal(got["O"][:40], alone["O"][:40]) and torch.equal(got["dQ"][:40], alone["dQ"][:40])
    assert bool(torch.isfinite(got["lse"][:40]).all()) and bool((got["lse"][40:] == float("-inf")).all())


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (True, True, True)], ids=str)
def test_unrequested_outputs_and_canaries(want):
    """The layout of tests/test_attn_grad_gpu.py: three gradients in one canary-filled allocation, rows of no view and of no group around the written spans."""
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
    with bf16():
        _lib.check(lib.must3r_hip_attn_grad(C.byref(a), C.c_void_p(scratch.data_ptr()), nb, C.c_void_p(_lib.stream_ptr(torch.device(DEV)))))
        full = TA.attention_grad(q, k, v, dO, tab, heads)
    torch.cuda.synchronize()
    written = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    span = dict(dQ=(5, 75), dK=(3, 73), dV=(3, 73))
    for n, w in zip(sizes, want):
        if w:
            written[off[n] + span[n][0] * D:off[n] + span[n][1] * D] = True
    assert bool((buf[~written] == CANARY).all()), "a float outside the requested outputs' rows was written"
    assert bool((buf[written] != CANARY).all()) and bool(torch.isfinite(buf[written]).all()), "a requested output was not written completely"
    for n, w, f in zip(sizes, want, full):
        if w:
            lo, hi = span[n]
            assert torch.equal(buf[off[n]:off[n] + sizes[n]].view(-1, D)[lo:hi], f[lo:hi]), n


def test_forward_leaves_rows_of_no_view_and_row_padding_alone():
    """O with a row stride of D + 4 inside a canary-filled buffer, q with NaN in its padding: rows [0, 5) and [45, 50) belong to no view."""
    lib = _lib.load()
    heads, D = 2, 128
    tab = torch.tensor([[5, 40, 0, 70, 10, 20]], dtype=torch.int32)
    g = torch.Generator().manual_seed(22)
    q, k, v = (torch.randn((R, D), generator=g).to(DEV) for R in (50, 70, 70))
    qbuf = torch.full((50, D + 4), float("nan"), device=DEV)
    qbuf[:, :D] = q
    obuf, lse = torch.full((50, D + 4), CANARY, device=DEV), torch.full((50, heads), CANARY, device=DEV)
    a = TA._args(qbuf[:, :D], k, v, tab, heads)
    a.O, a.ldo, a.lse = C.c_void_p(obuf.data_ptr()), D + 4, C.c_void_p(lse.data_ptr())
    scratch, nb = TA._scratch(tab, heads, q.device)
    with bf16():
        _lib.check(lib.must3r_hip_attn_forward_f32(C.byref(a), C.c_void_p(scratch.data_ptr()), nb, C.c_void_p(_lib.stream_ptr(torch.device(DEV)))))
        ref = TA.attention_forward(q, k, v, tab, heads)
    torch.cuda.synchronize()
    assert bool((obuf[:, D:] == CANARY).all()) and bool((obuf[:5] == CANARY).all()) and bool((obuf[45:] == CANARY).all())
    assert bool((lse[:5] == CANARY).all()) and bool((lse[45:] == CANARY).all()) and bool((lse[5:45] != CANARY).all())
    assert torch.equal(obuf[5:45, :D], ref[5:45]) and bool(torch.isfinite(ref[5:45]).all())


def test_fp32_mode_is_untouched_by_the_switch():
    d = _dev(_reference("cross_shared")[0])
    before = _gpu(d, mode=None)          # no context at all
    lib = _lib.load()
    for n in range(1, 4):
        for _ in range(n):
            lib.must3r_hip_train_attention_mode(1)
            lib.must3r_hip_train_attention_mode(0)
        _gpu(d)
        assert not _same(before, _gpu(d, mode="fp32")) and not _same(before, _gpu(d, mode=None))
    with TB.linear_precision("bf16"):          # the Linears' mode does not reach the core
        assert not _same(before, _gpu(d, mode=None))


# ---------------------------------------------------------------------------------------------------------------------------------
# a backward runs in the mode of its forward
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block_case(D, tokens, seed):
    return BR.make_case(D, D // 64, 4 * D, list(tokens), seed)


def _autograd(which, forward_in, backward_in, thread=False):
    if which == "attention":
        case = _reference("cross_shared")[0]
        d = _dev(case)
        leaves = [d[n].clone().requires_grad_(True) for n in ("q", "k", "v")]
        with TB.attention_precision(forward_in):
            out = TA.attention(*leaves, case["views"], case["heads"])
        up = d["dO"]
    elif which == "attention_f16_forward":
        case = _reference("cross_shared")[0]
        d = _dev(case)
        leaves = [d[n].clone().requires_grad_(True) for n in ("q", "k", "v")]
        with TB.attention_precision(forward_in):
            out = TA.attention(*leaves, case["views"], case["heads"], dtype=_lib.BF16)
        up = d["dO"]
    elif which == "attn":
        acase = _block_case(128, (70,), 31)
        leaves = [acase["x"].to(DEV).requires_grad_(True)] + [acase["params"][k].to(DEV).requires_grad_(True) for k in BR.ATTN_PARAMS]
        with TB.attention_precision(forward_in):
            out = TB.attention_sublayer(leaves[0], acase["pos"].to(DEV), acase["views"], 2, *leaves[1:], acase["rope"], acase["eps"])
        up = acase["dy"].to(DEV)
    else:
        ccase = DR.make_cross_case(128, 2, TA.memory_views(1, 2, 35, 0, mask=True), 70, 70, 72, False)
        leaves = [ccase["x"].to(DEV).requires_grad_(True), ccase["mem"].to(DEV).requires_grad_(True)] + \
                 [ccase["params"][k].to(DEV).requires_grad_(True) for k in DR.CROSS_PARAMS]
        with TB.attention_precision(forward_in):
            out = TC.cross_attention_sublayer(leaves[0], leaves[1], ccase["views"], 2, *leaves[2:], ccase["eps"])
        up = ccase["dy"].to(DEV)

    def back():
        with TB.attention_precision(backward_in):
            out.backward(up)
    if thread:
        t = threading.Thread(target=back)
        t.start()
        t.join()
    else:
        back()
    torch.cuda.synchronize()
    return [out.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("which", ["attention", "attn", "cross"])
def test_backward_runs_in_the_mode_of_its_forward(which):
    inside, outside, plain, mixed = (_autograd(which, *m) for m in (("bf16", "bf16"), ("bf16", None), (None, None), (None, "bf16")))
    assert all(torch.equal(s, t) for s, t in zip(inside, outside)), which
    assert all(torch.equal(s, t) for s, t in zip(plain, mixed)), which
    assert not torch.equal(inside[0], plain[0]) and not torch.equal(inside[1], plain[1]), which
    # on a thread of its own (which starts in the default mode), and inside the other mode's context
    assert all(torch.equal(s, t) for s, t in zip(inside, _autograd(which, "bf16", "fp32", thread=True))), which
    assert all(torch.equal(s, t) for s, t in zip(plain, _autograd(which, "fp32", "bf16", thread=True))), which


def test_the_16_bit_forward_keeps_its_meaning_and_its_backward_follows_the_mode():
    f32, b16 = _autograd("attention_f16_forward", None, None), _autograd("attention_f16_forward", "bf16", None)
    assert torch.equal(f32[0], b16[0])                                     # the native inference forward on cast operands, in either mode
    assert not torch.equal(f32[1], b16[1])                                 # its backward is must3r_hip_attn_grad in the mode of the forward
    assert all(torch.equal(s, t) for s, t in zip(b16[1:], _autograd("attention", "bf16", None)[1:]))


# ---------------------------------------------------------------------------------------------------------------------------------
# parity: sublayers and CachedDecoderBlock against fp64, the autocast run as the reference's own error
# ---------------------------------------------------------------------------------------------------------------------------------
def _autocast(fn):
    with torch.autocast("cpu", dtype=torch.bfloat16):
        res = fn()
    return {k: v.float() for k, v in res.items()}


SUB = {"d64_r19": (64, (19,), 41), "d128_r70": (128, (70,), 42)}


@functools.lru_cache(maxsize=None)
def _sub_reference(geom):
    case = _block_case(*SUB[geom])
    return BR.grads(case, torch.float64, "attn"), _autocast(lambda: BR.grads(case, torch.float32, "attn"))


@pytest.mark.parametrize("geom", list(SUB))
def test_attention_sublayer_matches_fp64_like_autocast(geom):
    case = _block_case(*SUB[geom])
    g64, gac = _sub_reference(geom)
    p = [case["params"][k].to(DEV) for k in BR.ATTN_PARAMS]
    x, dy = case["x"].to(DEV), case["dy"].to(DEV)
    pos, tab, rope = case["pos"].to(DEV), torch.tensor(case["views"], dtype=torch.int32), TB.rope_table(DEV, *case["rope"])
    with bf16():
        out, g = TB.attn_forward(x, pos, tab, rope, *p, case["eps"]), TB.attn_grad(x, pos, tab, rope, *p, dy, case["eps"])
    torch.cuda.synchronize()
    _compare(f"attn {geom} attn only", dict(zip(("out", "dx") + BR.ATTN_PARAMS, [out, *g])), g64, gac)


CROSS = {"d64_r19": (64, [[0, 19, 0, 89, 70, 89]], 19, 89, 43), "d128_r70": (128, TA.memory_views(1, 2, 35, 70, mask=True), 70, 140, 44)}
CROSS_VIEW_MASK = {"d64_r19": [0], "d128_r70": [0, 1]}


@functools.lru_cache(maxsize=None)
def _cross_case(geom):
    D, views, M, Rm, seed = CROSS[geom]
    return DR.make_cross_case(D, D // 64, views, M, Rm, seed, False)


@functools.lru_cache(maxsize=None)
def _cross_keep(geom):
    keep = torch.rand((2, CROSS[geom][3]), generator=torch.Generator().manual_seed(45)) < 0.7
    keep[:, :2] = True
    return keep


def _cross_keeps(geom, masked):
    return [_cross_keep(geom)[r] for r in CROSS_VIEW_MASK[geom]] if masked else None


@functools.lru_cache(maxsize=None)
def _cross_reference(geom, masked):
    case, extra = _cross_case(geom), {}
    g64 = DO.sublayer_grads(case, torch.float64, "cross", _cross_keeps(geom, masked), extra)
    return g64, _autocast(lambda: DO.sublayer_grads(case, torch.float32, "cross", _cross_keeps(geom, masked))), {KBIAS: extra["dK_colsum"]}


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "key_mask"])
@pytest.mark.parametrize("geom", list(CROSS))
def test_cross_sublayer_matches_fp64_like_autocast(geom, masked):
    case = _cross_case(geom)
    g64, gac, mags = _cross_reference(geom, masked)
    x, mem = case["x"].to(DEV).requires_grad_(True), case["mem"].to(DEV).requires_grad_(True)
    p = {k: case["params"][k].to(DEV).requires_grad_(True) for k in DR.param_names(case, "cross")}
    kw = dict(key_mask=TA.pack_key_mask(_cross_keep(geom).to(DEV)), view_mask=CROSS_VIEW_MASK[geom]) if masked else {}
    with bf16():
        out = TC.cross_attention_sublayer(x, mem, case["views"], case["heads"], *[p.get(k) for k in DR.CROSS_PARAMS], case["eps"], **kw)
    out.backward(case["dy"].to(DEV))          # after the block has ended
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dx=x.grad, dmem=mem.grad, **{k: t.grad for k, t in p.items()})
    assert set(got) == set(g64)
    _compare(f"cross {geom}{' key mask' if masked else ''} attn only", got, g64, gac, mags)


BLOCK = (128, 2, 512, 2, 2, 35, 70, 81)          # D, heads, hidden, scenes, V, n, Nm, seed: the d128 geometry of tests/test_cross_grad_gpu.py


@functools.lru_cache(maxsize=None)
def _dblock_case(mode):
    return DR.make_block_case(*BLOCK, mode=mode)


@functools.lru_cache(maxsize=None)
def _dblock_reference(mode):
    extra = {}
    g64 = DR.grads(_dblock_case(mode), torch.float64, "block", extra)
    return g64, _autocast(lambda: DR.grads(_dblock_case(mode), torch.float32, "block")), ({KBIAS: extra["dK_colsum"]} if mode != "kv" else None)


@pytest.mark.parametrize("mode", DR.MODES)
def test_decoder_block_matches_fp64_like_autocast(mode):
    case = _dblock_case(mode)
    g64, gac, mags = _dblock_reference(mode)
    blk = TC.CachedDecoderBlock(case["D"], case["heads"], case["hidden"] / case["D"], case["mode"], case["rope"], case["eps"])
    blk.load_state_dict(case["params"], strict=True)
    blk = blk.to(DEV)
    x, mem = case["x"].to(DEV).requires_grad_(True), case["mem"].to(DEV).requires_grad_(True)
    with bf16():
        y = TC.memory_rows(mem, blk.prepare_y(x), case["scenes"])
        out = blk(x, y, case["pos"].to(DEV), case["self_views"], case["views"])
    out.backward(case["dy"].to(DEV))
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dx=x.grad, dmem=mem.grad, **{k: t.grad for k, t in blk.named_parameters()})
    assert set(got) == set(g64)
    _compare(f"block d128 {mode} attn only", got, g64, gac, mags)


# ---------------------------------------------------------------------------------------------------------------------------------
# parity: the decoder over the branch-covering schedule
# ---------------------------------------------------------------------------------------------------------------------------------
def _group(name):
    head = name.split(".")[0]
    return {"blocks_dec": "blocks", "feedback_layer": "feedback", "feedback_norm": "feedback", "norm_dec": "head", "head_dec": "head",
            "feat_embed_enc_to_dec": "embed", "image2_embed": "embed"}.get(head, head.rstrip("0123456789"))


def _compare_grouped(tag, got, g64, gac, mags):
    rows = []
    try:
        GP.compare(rows, tag, got, g64, gac, mags)
    finally:
        for r in rows:
            key = (tag, _group(r[1]))
            if key not in _worst or r[5] > _worst[key][5]:
                _worst[key] = (tag, f"{key[1]}: {r[1]}", *r[2:])


@functools.lru_cache(maxsize=None)
def _dec_case(causal):
    return DF.make_case(mode="norm_y", causal=causal)          # B 2, views of 5 x 7 tokens, D 64, depth 3, single_mlp


@functools.lru_cache(maxsize=None)
def _dec_reference(causal):
    extra = {}
    g64 = DF.grads(_dec_case(causal), torch.float64, "pointmaps", extra)
    return g64, _autocast(lambda: DF.grads(_dec_case(causal), torch.float32, "pointmaps")), extra


def _dec_module(case):
    cls = TD.CausalMUSt3R if case["causal"] else TD.MUSt3R
    dec = cls(enc_embed_dim=case["Denc"], embed_dim=case["D"], depth=case["depth"], num_heads=case["heads"], mlp_ratio=case["hidden"] / case["D"],
              feedback_type=case["feedback_type"], memory_mode=case["mode"], rope=case["rope"], eps=case["eps"])
    dec.load_state_dict(case["params"], strict=True)
    return dec.to(DEV)


def _dec_run(case, dec, context, backward_inside=False):
    dec.zero_grad(set_to_none=True)
    xs = [c["x"].to(DEV).requires_grad_(True) for c in case["calls"]]
    B, n = case["scenes"], case["n"]
    mem, loss, res = None, 0, {}
    with context():
        for i, (c, x) in enumerate(zip(case["calls"], xs)):
            pos = case["pos"].to(DEV).view(1, 1, n, 2).expand(B, c["V"], n, 2).contiguous()
            ts = torch.tensor([case["H"], case["W"]]).view(1, 1, 2).expand(B, c["V"], 2).contiguous()
            mem, pts, tok = dec(x, pos, ts, mem, render=c["render"], return_tokens=True)
            res[f"tokens{i}"] = tok.detach().reshape(-1, case["D"])
            loss = loss + (pts * c["G"].to(DEV)).sum()
        if backward_inside:
            loss.backward()
    if not backward_inside:
        loss.backward()          # after the block has ended
    torch.cuda.synchronize()
    res.update({f"mem{l}": m.detach() for l, m in enumerate(mem[0])})
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    res.update({k: t.grad for k, t in dec.named_parameters()})
    return res


CONTEXTS = {"attn only": bf16, "amp": functools.partial(TB.amp, "bf16")}


@pytest.mark.parametrize("context", list(CONTEXTS))
@pytest.mark.parametrize("causal", [False, True], ids=["must3r", "causal"])
def test_decoder_matches_fp64_like_autocast_over_the_schedule(causal, context):
    case = _dec_case(causal)
    g64, gac, extra = _dec_reference(causal)
    dec = _dec_module(case)
    got = _dec_run(case, dec, CONTEXTS[context])
    names = [k for k in g64 if not k.startswith(("pointmaps", "feats"))]
    assert set(names) <= set(got)
    _compare_grouped(f"decoder {'causal' if causal else 'must3r'} {context}", got, {k: g64[k] for k in names}, gac, dict(extra))
    inside = _dec_run(case, dec, CONTEXTS[context], backward_inside=True)
    assert not [k for k in got if not torch.equal(got[k], inside[k])]
    other = _dec_run(case, dec, functools.partial(TB.linear_precision, "bf16" if context == "amp" else None))          # the same Linears, the fp32 core
    assert not torch.equal(other["tokens0"], got["tokens0"]) and not torch.equal(other["dx0"], got["dx0"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the caller's stream
# ---------------------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_run_on_the_callers_stream():
    """The harness of tests/test_stream_order_gpu.py (its delay, its bound case with the decoy inputs) on the cases attn_forward_f32 and attn_grad of
    tests/stream_forms.py, unchanged, in bf16 mode: the call is queued behind a delay on a side stream while its inputs hold the decoy, and there is no host
    wait between the queueing and the check that the delay is still running."""
    import stream_forms as SF
    import test_stream_order_gpu as SO
    delay = SO.Delay()
    for name in ("attn_forward_f32", "attn_grad"):
        with bf16():
            b = SO.Bound(SF.CASE[name])
            ref_a, ref_a2, ref_b = b.reference("A"), b.reference("A"), b.reference("B")
            assert not SO.same_bits(ref_a, ref_a2) and SO.differing_fraction(ref_a, ref_b) > 0.5
            b.load("B")
            b.fill()
            torch.cuda.synchronize()
            s = delay.side_stream()
            done = torch.cuda.Event()
            with torch.cuda.stream(s):
                delay.enqueue(40.0)
                done.record()
                b.load("A")
                outs = b.call()
                premise = not done.query()
                got = {k: v.clone() for k, v in outs.items()}
                b.load("B")
                b.fill()
            s.synchronize()
            assert premise, f"{name}: the delay ended before the call was queued"
            assert not SO.same_bits(got, ref_a), name
        with TB.attention_precision("fp32"):
            assert SO.same_bits(b.reference("A"), ref_a), f"{name}: the case did not run the bf16 kernels"
