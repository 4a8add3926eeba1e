"""GPU (-m gpu): the transformer block's training forward and backward -- csrc/train_block.hip through must3r_amd.train_block -- against the yardstick
tests/block_ref.py under CPU autograd, fed the same fp32 inputs in fp64 (truth) and in fp32 (the reference's own precision).

Parity is the rule of tests/test_loss_grad_gpu.py, tests/test_head_grad_gpu.py and tests/test_attn_grad_gpu.py, unchanged: per case and tensor,
``e_gpu`` = max |GPU - fp64|, ``e_ref`` = max |fp32 CPU autograd - fp64|, required ``e_gpu <= 4 e_ref + 32 2^-24 max|g64|``; forward outputs are held to
it like gradients.  Every row is printed before it is asserted and goes, as a table, to the file M3R_BLOCK_GRAD_TABLE names (kept as
profiles/block_grad_parity.txt).  The upstream gradient is of order 1e-7.

The activation alone is held to a bound of its own, from the arithmetic: the argument of erfc and of exp carries one rounding, which the tails amplify by
z^2 (d ln Phi / d ln z and d ln phi / d ln z are of that order), so an error of (2 z^2 + 32) 2^-24 relative to |z| Phi(z) (gelu) and to Phi(z) + |z| phi(z)
(gelu', whose two terms cancel near z = -0.75) is allowed.

The exact conditions (determinism, a view alone against the view in a batch, linearity, outputs that were not asked for, canaries, untouched value columns) have
no tolerance.
"""
import ctypes as C
import functools
import math
import os

import pytest
import torch

import block_ref as BR
import grad_parity as GP
from must3r_amd import _lib, train_block as TB

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
CANARY = -7.25e11
_rows = []

# D, heads, hidden, tokens per view, seed: a key tile plus a tail, one exact tile and one all-tail view; the decoder's and the encoder's geometry
GEOMS = {"d128_ragged": (128, 2, 512, (70, 64, 17), 41), "d768": (768, 12, 3072, (96, 96), 42), "d1024": (1024, 16, 4096, (96, 96), 43)}

_HEADER = (
    "# tests/test_block_grad_gpu.py: per case and tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in units of",
    "# 2^-24 max|g64|; bound = 4 e_ref + 32; ratio = e_gpu / bound.  Forward outputs are held to the same bound.  The two gelu rows are pointwise:",
    "# the worst point of the grid, e_gpu in units of 2^-24 |z| Phi (gelu) or 2^-24 (Phi + |z| phi) (gelu'), bound (2 z^2 + 32) of those units.",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_BLOCK_GRAD_TABLE"), _HEADER, _rows, (30, 18))


_compare = functools.partial(GP.compare, _rows)


@functools.lru_cache(maxsize=None)
def _case(geom):
    D, heads, hidden, tokens, seed = GEOMS[geom]
    return BR.make_case(D, heads, hidden, list(tokens), seed)


@functools.lru_cache(maxsize=None)
def _reference(geom, which):
    """(fp64 results, fp32 results): computed once, shared, never modified."""
    return BR.grads(_case(geom), torch.float64, which), BR.grads(_case(geom), torch.float32, which)


def _dev(case):
    d = dict(case)
    d.update(x=case["x"].to(DEV), dy=case["dy"].to(DEV), pos=case["pos"].to(DEV), tab=torch.tensor(case["views"], dtype=torch.int32),
             params={k: v.to(DEV) for k, v in case["params"].items()}, rope_tab=TB.rope_table(DEV, *case["rope"]))
    return d


def _mlp(d, dy=None, want=(True,) * 7, x=None):
    p = [d["params"][k] for k in BR.MLP_PARAMS]
    x = d["x"] if x is None else x
    out = TB.mlp_forward(x, *p, d["eps"])
    g = TB.mlp_grad(x, *p, d["dy"] if dy is None else dy, d["eps"], want=want)
    torch.cuda.synchronize()
    return dict(zip(("out", "dx") + BR.MLP_PARAMS, [out, *g]))


def _attn(d, dy=None, want=(True,) * 7, rows=None, views=None):
    p = [d["params"][k] for k in BR.ATTN_PARAMS]
    sl = slice(None) if rows is None else rows
    x, pos, dy = d["x"][sl].contiguous(), d["pos"][sl].contiguous(), (d["dy"] if dy is None else dy)[sl].contiguous()
    tab = d["tab"] if views is None else torch.tensor(views, dtype=torch.int32)
    out = TB.attn_forward(x, pos, tab, d["rope_tab"], *p, d["eps"])
    g = TB.attn_grad(x, pos, tab, d["rope_tab"], *p, dy, d["eps"], want=want)
    torch.cuda.synchronize()
    return dict(zip(("out", "dx") + BR.ATTN_PARAMS, [out, *g]))


def _module(case):
    blk = TB.Block(case["D"], case["heads"], case["hidden"] / case["D"], case["rope"], case["eps"])
    blk.load_state_dict(case["params"], strict=True)
    return blk.to(DEV)


def _block(d, dy=None, rows=None, views=None, blk=None):
    """The block through the module and torch.autograd."""
    blk = _module(d) if blk is None else blk
    blk.zero_grad(set_to_none=True)
    sl = slice(None) if rows is None else rows
    x = d["x"][sl].clone().requires_grad_(True)
    out = blk(x, d["pos"][sl], d["views"] if views is None else views)
    out.backward((d["dy"] if dy is None else dy)[sl])
    torch.cuda.synchronize()
    res = dict(out=out.detach(), dx=x.grad)
    res.update({k: t.grad for k, t in blk.named_parameters()})
    return res


RUN = {"mlp": _mlp, "attn": _attn, "block": _block}


# ---------------------------------------------------------------------------------------------------------------------------------
# the operators
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,lda", [(150, 192, 128, 160), (6, 64, 64, 64)], ids=["tile_plus_tails", "all_tail"])
def test_linear_three_epilogues(M, N, K, lda):
    """150 x 192 x 128: one 128-tile and a tail in both directions, a leading dimension larger than K; 6 x 64 x 64: all tail."""
    g = torch.Generator().manual_seed(51)
    a, w, b, res = torch.randn((M, lda), generator=g), torch.randn((N, K), generator=g) * K ** -0.5, torch.randn(N, generator=g), torch.randn((M, N), generator=g)
    ref = {}
    for dt in (torch.float64, torch.float32):
        z = a[:, :K].to(dt) @ w.to(dt).t() + b.to(dt)
        ref[dt] = dict(bias=z, bias_res=res.to(dt) + z, gelu=0.5 * z * (1 + torch.erf(z * 2 ** -0.5)), z=z)
    ad, wd, bd, rd = a.to(DEV)[:, :K], w.to(DEV), b.to(DEV), res.to(DEV)
    assert ad.stride(0) == lda
    h, z = TB.linear_forward(ad, wd, bd, _lib.LIN_BIAS_GELU, want_z=True)
    got = dict(bias=TB.linear_forward(ad, wd, bd), bias_res=TB.linear_forward(ad, wd, bd, _lib.LIN_BIAS_RES, res=rd), gelu=h, z=z)
    _compare(f"linear {M}x{N}x{K}", got, ref[torch.float64], ref[torch.float32])
    assert torch.equal(got["z"], got["bias"]) and torch.equal(TB.linear_forward(ad, wd, bd, _lib.LIN_BIAS_GELU), h)
    # the residual may be the output buffer
    out = rd.clone()
    TB.linear_forward(ad, wd, bd, _lib.LIN_BIAS_RES, res=out, out=out)
    assert torch.equal(out, got["bias_res"])
    # tails are not stored: the output is the middle of a canary-filled buffer
    buf = torch.full((M + 2, N), CANARY, device=DEV)
    TB.linear_forward(ad, wd, bd, out=buf[1:M + 1])
    assert torch.equal(buf[1:M + 1], got["bias"]) and bool((buf[0] == CANARY).all()) and bool((buf[M + 1] == CANARY).all())
    assert torch.equal(TB.linear_forward(ad, wd, None), TB.linear_forward(ad, wd, torch.zeros_like(bd)))


def test_gelu_and_its_derivative():
    z = torch.cat([torch.linspace(-12, 12, 4801), torch.tensor([40.0, -40.0, 1e4, -1e4, 3.4e38, -3.4e38, 0.0])])
    g, dg = TB.gelu_eval(z.to(DEV))
    g, dg = g.cpu(), dg.cpu()
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(dg).all())
    # the exact limits
    assert dg[4801:4807].tolist() == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0] and float(dg[-1]) == 0.5
    assert g[4801:4807].tolist() == [40.0, 0.0, 1e4, 0.0, float(torch.tensor(3.4e38)), 0.0] and float(g[-1]) == 0.0
    assert bool((dg[z >= 40] == 1).all()) and bool((dg[z <= -40] == 0).all())
    z64 = z[:4801].double()
    cdf, pdf = 0.5 * torch.erfc(-z64 / math.sqrt(2)), torch.exp(-0.5 * z64 * z64) / math.sqrt(2 * math.pi)
    tol = (2 * z64 * z64 + 32) * U
    e_g, b_g = (g[:4801].double() - z64 * cdf).abs(), tol * (z64 * cdf).abs() + 1e-44
    e_d, b_d = (dg[:4801].double() - (cdf + z64 * pdf)).abs(), tol * (cdf + z64.abs() * pdf)
    for name, e, b, ref in (("gelu", e_g, b_g, z64 * cdf), ("gelu'", e_d, b_d, cdf + z64 * pdf)):
        i = int((e / b).argmax())      # the table's row: the point of the worst error / bound, its error in units of 2^-24 of the condition-aware magnitude
        _rows.append(("gelu pointwise [-12, 12]", f"{name} z={float(z64[i]):.3f}", float(ref.abs().max()), float(e[i] / (b[i] / tol[i] * U)), float("nan"),
                      float(e[i] / b[i])))
        print(f"{name}: worst error / bound {float(e[i] / b[i]):.3f} at z = {float(z64[i]):.4f}")
    assert bool((e_g <= b_g).all()) and bool((e_d <= b_d).all())
    # gelu_grad: dh gelu'(z) over row-strided tensors, in place
    zz = torch.randn((70, 136), generator=torch.Generator().manual_seed(52)).to(DEV) * 3
    dh = torch.randn((70, 136), generator=torch.Generator().manual_seed(53)).to(DEV)
    want = dh[:, :132] * TB.gelu_eval(zz[:, :132].contiguous(), want=(False, True))[1]
    assert torch.equal(TB.gelu_grad(dh[:, :132], zz[:, :132]), want)
    buf = dh.clone()
    TB.gelu_grad(buf[:, :132], zz[:, :132], out=buf[:, :132])
    assert torch.equal(buf[:, :132], want) and torch.equal(buf[:, 132:], dh[:, 132:])


def test_rope_both_directions():
    """Rows of 3 D = 384 floats, the first 2 D rotated: forward against the oracle's rope2d, the transpose against its autograd."""
    R_, D, heads = 151, 128, 2
    g = torch.Generator().manual_seed(54)
    t = torch.randn((R_, 3 * D), generator=g)
    pos = torch.stack([torch.randint(0, 40, (R_,), generator=g), torch.randint(0, 40, (R_,), generator=g)], dim=1)
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaf = t[:, :2 * D].to(dt).clone().requires_grad_(True)
        fwd = torch.cat([BR.rope_rows(leaf[:, :D], pos, heads, (100.0, 1.0)), BR.rope_rows(leaf[:, D:], pos, heads, (100.0, 1.0))], dim=1)
        fwd.backward(t[:, :2 * D].to(dt))
        ref[dt] = dict(forward=fwd.detach(), transpose=leaf.grad)
    tab = TB.rope_table(DEV)
    assert TB.rope_table(DEV) is tab and tab.shape == (256, 16, 2)
    cos, sin = BR.R.rope_tables(256)
    assert torch.allclose(tab[..., 0].cpu(), cos, rtol=0, atol=4 * U) and torch.allclose(tab[..., 1].cpu(), sin, rtol=0, atol=4 * U)    # two roundings of cosf / sinf apart
    td, pd = t.to(DEV), pos.to(DEV)
    f, b = td.clone(), td.clone()
    TB.rope_rows(f, pd, tab, 2 * D, 1)
    TB.rope_rows(b, pd, tab, 2 * D, -1)
    _compare("rope 151x384", dict(forward=f[:, :2 * D], transpose=b[:, :2 * D]), ref[torch.float64], ref[torch.float32])
    assert torch.equal(f[:, 2 * D:], td[:, 2 * D:]) and torch.equal(b[:, 2 * D:], td[:, 2 * D:])          # the value columns, bit for bit
    TB.rope_rows(f, pd, tab, 2 * D, -1)
    # a rotation and its transpose: three roundings per element and cos^2 + sin^2 = 1 to two roundings, on pairs of magnitude at most sqrt 2 max|t|
    assert float((f - td).abs().max()) <= 8 * U * float(td.abs().max())
    # a position past the table is refused where Python can see it
    case = _dev(_case("d128_ragged"))
    bad = case["pos"].clone()
    bad[3, 1] = 256
    with pytest.raises(ValueError, match="position"):
        TB.attention_sublayer(case["x"], bad, case["views"], 2, *[case["params"][k] for k in BR.ATTN_PARAMS])


@pytest.mark.parametrize("D", [128, 1024])
def test_layernorm_backward_with_add(D):
    M = 70
    g = torch.Generator().manual_seed(55 + D)
    x, gamma, beta = torch.randn((M, D), generator=g), 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy, add = torch.randn((M, D), generator=g) * 1e-7, torch.randn((M, D), generator=g) * 1e-7
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = [v.to(dt).clone().requires_grad_(True) for v in (x, gamma, beta)]
        y = BR.R.layer_norm(*leaves, 1e-6)
        y.backward(dy.to(dt))
        ref[dt] = dict(y=y.detach(), dx=leaves[0].grad + add.to(dt), dgamma=leaves[1].grad, dbeta=leaves[2].grad)
    xd, gd, bd, dyd, addd = (v.to(DEV) for v in (x, gamma, beta, dy, add))
    dx, dg, db = TB.layernorm_grad(xd, gd, dyd, 1e-6, add=addd)
    _compare(f"layernorm_grad_add D{D}", dict(y=TB.layernorm_forward(xd, gd, bd, 1e-6), dx=dx, dgamma=dg, dbeta=db), ref[torch.float64], ref[torch.float32])
    # the entry point without add: equal to a run of itself, and to the new entry point given zeros
    a, b = TB.layernorm_grad(xd, gd, dyd, 1e-6), TB.layernorm_grad(xd, gd, dyd, 1e-6)
    z = TB.layernorm_grad(xd, gd, dyd, 1e-6, add=torch.zeros_like(addd))
    for u, v, w in zip(a, b, z):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert torch.equal(dg, a[1]) and torch.equal(db, a[2])
    # in place over dy, with add the output buffer of another call
    buf = dyd.clone()
    lib = _lib.load()
    nb = lib.must3r_hip_op_layernorm_grad_scratch_bytes(M, D)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    P = lambda v: C.c_void_p(v.data_ptr())
    _lib.check(lib.must3r_hip_op_layernorm_grad_add(P(xd), P(gd), P(buf), P(addd), P(buf), None, None, M, D, 1e-6, P(scratch), nb,
                                                    C.c_void_p(_lib.stream_ptr(torch.device(DEV)))))
    torch.cuda.synchronize()
    assert torch.equal(buf, dx)


def test_linear_and_layer_norm_autograd():
    g = torch.Generator().manual_seed(56)
    x, w, b, dy = torch.randn((2, 35, 128), generator=g), torch.randn((192, 128), generator=g) * 0.1, torch.randn(192, generator=g), torch.randn((2, 35, 192), generator=g) * 1e-7
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = [v.to(dt).clone().requires_grad_(True) for v in (x, w, b)]
        out = leaves[0] @ leaves[1].t() + leaves[2]
        out.backward(dy.to(dt))
        ref[dt] = dict(out=out.detach(), dx=leaves[0].grad, dW=leaves[1].grad, db=leaves[2].grad)
    leaves = [v.to(DEV).requires_grad_(True) for v in (x, w, b)]
    out = TB.linear(*leaves)
    out.backward(dy.to(DEV))
    _compare("linear autograd 70x192x128", dict(out=out, dx=leaves[0].grad, dW=leaves[1].grad, db=leaves[2].grad), ref[torch.float64], ref[torch.float32])
    xs = x.to(DEV).half().requires_grad_(True)
    gam = torch.ones(128, device=DEV, requires_grad=True)
    y = TB.layer_norm(xs, gam, torch.zeros(128, device=DEV))
    y.sum().backward()
    assert y.dtype == torch.float32 and xs.grad.dtype == torch.float16 and xs.grad.shape == xs.shape and gam.grad.shape == (128,)


# ---------------------------------------------------------------------------------------------------------------------------------
# the sublayers and the block: parity
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mlp", "attn", "block"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_forward_and_gradients_match_autograd(geom, which):
    g64, g32 = _reference(geom, which)
    got = RUN[which](_dev(_case(geom)))
    _compare(f"{which} {geom}", got, g64, g32)


def test_direct_calls_equal_the_module():
    """The block through autograd is the two sublayer entry points chained: the same bits."""
    d = _dev(_case("d128_ragged"))
    blk = _block(d)
    a = _attn(d)
    m = _mlp(d, x=a["out"])
    assert torch.equal(m["out"], blk["out"])
    a2 = _attn(d, dy=m["dx"])
    for k in BR.MLP_PARAMS:
        assert torch.equal(m[k], blk[k]), k
    for k in ("dx",) + BR.ATTN_PARAMS:
        assert torch.equal(a2[k], blk[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# exact conditions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mlp", "attn", "block"])
def test_calls_repeat_bitwise(which):
    d = _dev(_case("d128_ragged"))
    a, b = RUN[which](d), RUN[which](d)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_view_alone_equals_view_in_batch():
    """A view's rows of the output and of dx are the same bits alone and inside the batch of three."""
    case = _case("d128_ragged")
    d = _dev(case)
    blk = _module(case)
    full = _block(d, blk=blk)
    full_attn = _attn(d)
    for i, (r0, n, _, _, _, _) in enumerate(case["views"]):
        rows = slice(r0, r0 + n)
        one = _block(d, rows=rows, views=[[0, n, 0, n, 0, 0]], blk=blk)
        assert torch.equal(one["out"], full["out"][rows]) and torch.equal(one["dx"], full["dx"][rows]), i
        one = _attn(d, rows=rows, views=[[0, n, 0, n, 0, 0]])
        assert torch.equal(one["out"], full_attn["out"][rows]) and torch.equal(one["dx"], full_attn["dx"][rows]), i


@pytest.mark.parametrize("which", ["mlp", "attn", "block"])
def test_backward_is_linear_in_the_upstream_gradient(which):
    d = _dev(_case("d128_ragged"))
    a, b = RUN[which](d), RUN[which](d, dy=d["dy"] * 2)
    for k in a:
        if k != "out":
            assert torch.equal(a[k] * 2, b[k]), k


WANTS = {"all": (True,) * 7, "frozen_norms": (True, False, False, True, True, True, True), "frozen_weights": (True, True, True, False, False, False, False),
         "frozen_x": (False, True, True, True, True, True, True), "x_only": (True,) + (False,) * 6, "last_linear_only": (False,) * 5 + (True, True),
         "biases_only": (False, False, True, False, True, False, True), "last_bias_only": (False,) * 6 + (True,)}


@pytest.mark.parametrize("want", list(WANTS))
@pytest.mark.parametrize("which", ["mlp", "attn"])
def test_unrequested_outputs_and_canaries(which, want):
    """The seven gradients lie in one canary-filled allocation with 64 canaries around each.  An output that is not asked for is NULL; its floats and every
    canary must survive, the rest is written completely and equals the full run bit for bit."""
    lib = _lib.load()
    d = _dev(_case("d128_ragged"))
    M, D, Hd, PAD = d["M"], d["D"], d["hidden"], 64
    full = RUN[which](d)
    if which == "mlp":
        names, fields, a = BR.MLP_PARAMS, TB.MLP_OUTPUTS, TB._mlp_args(d["x"], *[d["params"][k] for k in BR.MLP_PARAMS], d["eps"])
        sizes = [M * D, D, D, Hd * D, Hd, D * Hd, D]
        nb, fn = lib.must3r_hip_mlp_sublayer_scratch_bytes(M, D, Hd), lib.must3r_hip_mlp_sublayer_grad
    else:
        names, fields = BR.ATTN_PARAMS, TB.ATTN_OUTPUTS
        a = TB._attn_args(d["x"], d["pos"], d["tab"], d["rope_tab"], *[d["params"][k] for k in BR.ATTN_PARAMS], d["eps"])
        sizes = [M * D, D, D, 3 * D * D, 3 * D, D * D, D]
        nb, fn = lib.must3r_hip_attn_sublayer_scratch_bytes(M, D, len(d["views"])), lib.must3r_hip_attn_sublayer_grad
    buf = torch.full((sum(sizes) + PAD * (len(sizes) + 1),), CANARY, device=DEV)
    off, o = [], PAD
    for s in sizes:
        off.append(o)
        o += s + PAD
    a.dy = C.c_void_p(d["dy"].data_ptr())
    for f, w, o in zip(fields, WANTS[want], off):
        setattr(a, f, C.c_void_p(buf.data_ptr() + 4 * o) if w else None)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(fn(C.byref(a), C.c_void_p(scratch.data_ptr()), nb, C.c_void_p(_lib.stream_ptr(torch.device(DEV)))))
    torch.cuda.synchronize()
    written = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    for n, w, o, s in zip(("dx",) + names, WANTS[want], off, sizes):
        if w:
            written[o:o + s] = True
            assert torch.equal(buf[o:o + s], full[n].reshape(-1)), n
    assert bool((buf[~written] == CANARY).all()), "a float outside the requested outputs was written"


@pytest.mark.parametrize("frozen", ["norms", "weights", "x"])
def test_needs_input_grad_combinations(frozen):
    d = _dev(_case("d128_ragged"))
    full = _block(d)
    blk = _module(d)
    for k, t in blk.named_parameters():
        if (frozen == "norms" and k.startswith("norm")) or (frozen == "weights" and not k.startswith("norm")):
            t.requires_grad_(False)
    x = d["x"].clone().requires_grad_(frozen != "x")
    blk(x, d["pos"], d["views"]).backward(d["dy"])
    assert (x.grad is None) == (frozen == "x")
    if frozen != "x":
        assert torch.equal(x.grad, full["dx"])
    for k, t in blk.named_parameters():
        assert (t.grad is None) == (not t.requires_grad), k
        if t.requires_grad:
            assert t.grad.dtype == t.dtype and t.grad.shape == t.shape and torch.equal(t.grad, full[k]), k


def test_rows_of_no_view_attend_nothing():
    """Rows [0, 5) and [75, 80) belong to no view: out = x + proj.bias there, and dx = dy."""
    d = _dev(_case("d128_ragged"))
    rows, views = slice(0, 80), [[5, 40, 5, 40, 0, 0], [45, 30, 45, 30, 0, 0]]
    got = _attn(d, rows=rows, views=views)
    for sl in (slice(0, 5), slice(75, 80)):
        assert torch.equal(got["out"][sl], d["x"][rows][sl] + d["params"]["attn.proj.bias"]) and torch.equal(got["dx"][sl], d["dy"][rows][sl])
    one = _attn(d, rows=slice(5, 45), views=[[0, 40, 0, 40, 0, 0]])
    assert torch.equal(one["out"], got["out"][5:45]) and torch.equal(one["dx"], got["dx"][5:45])


def test_optimizer_step_is_seen_by_the_next_forward():
    case = _case("d128_ragged")
    d = _dev(case)
    blk = _module(case)
    opt = torch.optim.SGD(blk.parameters(), lr=1e4)
    x = d["x"].view(1, -1, case["D"])
    before = blk(x, d["pos"].view(1, -1, 2), d["views"])
    assert before.shape == x.shape
    before.backward(d["dy"].view(x.shape))
    opt.step()
    after = blk(x, d["pos"].view(1, -1, 2), d["views"])
    fresh = TB.Block(case["D"], case["heads"], case["hidden"] / case["D"]).to(DEV)
    fresh.load_state_dict(blk.state_dict())
    assert not torch.equal(after, before) and torch.equal(after, fresh(x, d["pos"].view(1, -1, 2), d["views"]))
    # [B, N, D] with the default table: one view per batch entry
    xb = d["x"][:128].view(2, 64, case["D"])
    assert torch.equal(blk(xb, d["pos"][:128].view(2, 64, 2)).view(128, -1), blk(d["x"][:128], d["pos"][:128], [[0, 64, 0, 64, 0, 0], [64, 64, 64, 64, 0, 0]]))


@pytest.mark.parametrize("which", ["x", "weight"])
def test_in_place_change_of_a_saved_input_raises(which):
    d = _dev(_case("d128_ragged"))
    blk = _module(d)
    x = d["x"].clone().requires_grad_(True)
    xin = x * 1.0
    out = blk(xin, d["pos"], d["views"])
    with torch.no_grad():
        (xin if which == "x" else blk.mlp.fc1.weight).mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward(d["dy"])
