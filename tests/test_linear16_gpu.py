"""GPU (-m gpu): the training Linears on the 16-bit MFMA (csrc/train_lin16.hip) and the switch that selects them (must3r_hip_train_linear_mode through
``train_block.linear_precision``).

The operator forms are held to the exact-operand reference tests/linear16_ref.py: with both operands rounded to bf16 every product is exact in fp32, so

    |got - ref64| <= (K_c + 4) 2^-24 (sum_k |a^_k| |w^_k| + |bias| + |res|)        K_c = K (forward), O (dgrad), the row count (wgrad, db)

per element -- derived (one rounding per addition, whatever the order), not measured.  The GELU epilogue: z to that bound, gelu(z) to the fp64 GELU of the
GPU's own z within the pointwise tolerance of tests/test_block_grad_gpu.py, (2 z^2 + 32) 2^-24 |z| Phi(z).

The sublayers and the decoder are held by the project's parity rule (tests/grad_parity.py) with fp32 CPU autograd under ``torch.autocast("cpu", bfloat16)``
as the reference run: e_gpu <= 4 e_autocast + 32 2^-24 m against fp64.

Every row is printed before it is asserted and goes to the file M3R_LINEAR16_TABLE names (kept as profiles/linear16_parity.txt).  Exact conditions
(repeatability, a scene's rows alone, canaries, the segmented data gradient, the switch) have no tolerance.
"""
import ctypes as C
import functools
import math
import os
import threading

import pytest
import torch

import block_ref as BR
import decblock_ref as DR
import decoder_ref as DF
import dropout_ref as DO
import grad_parity as GP
import linear16_ref as LR
from must3r_amd import _lib, train_attention as TA, train_block as TB, train_cross as TC, train_decoder as TD, train_optim as TO

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
CANARY = -7.25e11
KBIAS = "cross_attn.projk.bias"
NAN = float("nan")
_rows = []

_HEADER = (
    "# tests/test_linear16_gpu.py, bf16 mode of the training Linears.  Operator rows (linear / dgrad / wgrad): the reference rounds the operands to bf16 and",
    "# sums in fp64; m = max of the element scale s = sum |a^||w^| + |bias| + |res|; e_gpu = worst |got - ref| in units of 2^-24 m; e_ref not applicable (nan);",
    "# ratio = worst over the elements of |got - ref| / ((K_c + 4) 2^-24 s), required <= 1.  The gelu rows: gelu(z) against the fp64 GELU of the GPU's z, ratio",
    "# to (2 z^2 + 32) 2^-24 |z| Phi(z).  Sublayer and decoder rows: e_gpu = max |GPU bf16 mode - fp64|, e_ref = max |fp32 CPU autograd under bf16 autocast - fp64|,",
    "# both in units of 2^-24 m; bound = 4 e_ref + 32; ratio = e_gpu / bound.  m = max|g64|, except for cross_attn.projk.bias (true gradient zero): the largest",
    "# column 1-norm of the fp64 dK.  Decoder rows: the worst tensor of each group.",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    _lib.load().must3r_hip_train_linear_mode(0)
    yield
    GP.write_table(os.environ.get("M3R_LINEAR16_TABLE"), _HEADER, _rows + list(_worst.values()), (34, 60), magnitude="m")


bf16 = functools.partial(TB.linear_precision, "bf16")


# ---------------------------------------------------------------------------------------------------------------------------------
# the operator forms through the C entry points (row strides and optional outputs as the sublayers pass them)
# ---------------------------------------------------------------------------------------------------------------------------------
def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def ld(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def padded(t, pad=4, fill=NAN):
    """t as the first columns of rows ``pad`` floats longer, the padding filled with NaN"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def dgrad(dz, W, out=None):
    M, O, K = int(dz.shape[0]), int(dz.shape[1]), int(W.shape[1])
    out = torch.empty((M, K), device=DEV) if out is None else out
    _lib.check(_lib.load().must3r_hip_op_linear_dgrad_f32(P(dz), ld(dz), P(W), P(out), M, O, K, ST()))
    return out


def wgrad(dz, a, dW, db):
    lib = _lib.load()
    R, O, K = int(dz.shape[0]), int(dz.shape[1]), int(a.shape[1])
    nb = lib.must3r_hip_op_linear_wgrad_scratch_bytes(R, O, K)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.must3r_hip_op_linear_wgrad_f32(P(dz), ld(dz), P(a) if dW is not None else None, ld(a), P(dW), P(db), R, O, K, P(scratch), nb, ST()))
    torch.cuda.synchronize()


def hold(tag, name, got, ref, scale, Kc):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (tag, name)
    err = (got - ref).abs()
    ratio = float((err / LR.bound(Kc, scale)).max())
    m = float(scale.max())
    _rows.append((tag, name, m, float(err.max()) / (U * m), NAN, ratio))
    print(f"{tag} {name}: K_c {Kc} worst |got - ref| / bound {ratio:.4f}")
    assert ratio <= 1.0, (tag, name, ratio)


# M, N, K, strided
FORWARD = [(1, 4, 16, False), (19, 68, 48, True), (70, 128, 64, False), (129, 192, 768, True), (300, 68, 16, True), (300, 192, 48, False)]


@pytest.mark.parametrize("M,N,K,strided", FORWARD)
def test_forward_three_epilogues(M, N, K, strided):
    a, w, b, res = LR.inputs(M, N, K, 21)
    tag = f"linear {M}x{N}x{K}" + (" ld K+4" if strided else "")
    ad, wd, bd, rd = (padded(a.to(DEV)) if strided else a.to(DEV)), w.to(DEV), b.to(DEV), (padded(res.to(DEV)) if strided else res.to(DEV))
    ref_b, sc_b = LR.forward(a, w, b)
    ref_r, sc_r = LR.forward(a, w, b, res)
    with bf16():
        got_b = TB.linear_forward(ad, wd, bd)
        got_r = TB.linear_forward(ad, wd, bd, _lib.LIN_BIAS_RES, res=rd)
        h, z = TB.linear_forward(ad, wd, bd, _lib.LIN_BIAS_GELU, want_z=True)
        hold(tag, "bias", got_b, ref_b, sc_b, K)
        hold(tag, "bias_res", got_r, ref_r, sc_r, K)
        hold(tag, "gelu z", z, ref_b, sc_b, K)
        z64 = z.cpu().double()
        g64 = z64 * 0.5 * torch.erfc(-z64 / math.sqrt(2))
        e, tol = (h.cpu().double() - g64).abs(), (2 * z64 * z64 + 32) * U * g64.abs() + 1e-44
        _rows.append((tag, "gelu(z)", float(g64.abs().max()), float(e.max()) / (U * float(g64.abs().max())), NAN, float((e / tol).max())))
        assert bool((e <= tol).all()), (tag, float((e / tol).max()))
        # the pre-activation is the bias epilogue's output; two calls give equal bits; without a bias: a bias of zeros
        assert torch.equal(z, got_b) and torch.equal(TB.linear_forward(ad, wd, bd), got_b) and torch.equal(TB.linear_forward(ad, wd, bd, _lib.LIN_BIAS_GELU), h)
        assert torch.equal(TB.linear_forward(ad, wd, None), TB.linear_forward(ad, wd, torch.zeros_like(bd)))
        # the residual may be the output buffer (a strided one: its NaN padding survives)
        out = padded(res.to(DEV)) if strided else res.to(DEV).clone()
        TB.linear_forward(ad, wd, bd, _lib.LIN_BIAS_RES, res=out, out=out)
        assert torch.equal(out, got_r)
        # tails are not stored, z is not written where it is not asked for
        buf = torch.full((M + 2, N), CANARY, device=DEV)
        TB.linear_forward(ad, wd, bd, out=buf[1:M + 1])
        assert torch.equal(buf[1:M + 1], got_b) and bool((buf[0] == CANARY).all()) and bool((buf[M + 1] == CANARY).all())
        # a block of rows alone has the bits of those rows in the batch
        r0, r1 = M // 3, M // 3 + max(1, M // 2)
        assert torch.equal(TB.linear_forward(ad[r0:r1], wd, bd), got_b[r0:r1])
    assert not torch.equal(TB.linear_forward(ad, wd, bd), got_b)        # outside the context: the fp32 form, which rounds nothing


# M, O (contraction), K (columns of dX), strided
DGRAD = [(1, 16, 4, False), (19, 48, 68, True), (70, 64, 128, False), (129, 768, 192, True), (300, 16, 68, True), (300, 48, 192, False)]


@pytest.mark.parametrize("M,O,K,strided", DGRAD)
def test_dgrad(M, O, K, strided):
    g = torch.Generator().manual_seed(22)
    dz, w = torch.randn((M, O), generator=g), torch.randn((O, K), generator=g) * O ** -0.5
    if M > 2:
        dz[1] *= 2.0 ** 20
        dz[M // 2] *= 2.0 ** -20
    dzd, wd = (padded(dz.to(DEV)) if strided else dz.to(DEV)), w.to(DEV)
    ref, scale = LR.dgrad(dz, w)
    with bf16():
        got = dgrad(dzd, wd)
        hold(f"dgrad {M}x{O}x{K}" + (" ld O+4" if strided else ""), "dX", got, ref, scale, O)
        assert torch.equal(dgrad(dzd, wd), got)
        buf = torch.full((M + 2, K), CANARY, device=DEV)
        dgrad(dzd, wd, out=buf[1:M + 1])
        assert torch.equal(buf[1:M + 1], got) and bool((buf[0] == CANARY).all()) and bool((buf[M + 1] == CANARY).all())
        r0, r1 = M // 3, M // 3 + max(1, M // 2)
        assert torch.equal(dgrad(dzd[r0:r1], wd), got[r0:r1])


# rows, O, K, strided: 2056 rows are 16 splits of 129 -> 144 rows, a length that is no multiple of the 32-deep step
WGRAD = [(1, 4, 16, False), (127, 68, 48, True), (129, 128, 64, False), (2049 + 7, 192, 128, True)]


@pytest.mark.parametrize("R,O,K,strided", WGRAD)
def test_wgrad_and_its_optional_outputs(R, O, K, strided):
    dz, a = LR.wgrad_inputs(R, O, K, 23)
    dzd, ad = ((padded(dz.to(DEV)), padded(a.to(DEV))) if strided else (dz.to(DEV), a.to(DEV)))
    rW, sW, rb, sb = LR.wgrad(dz, a)
    tag = f"wgrad {R}x{O}x{K}" + (" ld +4" if strided else "")
    PAD = 64
    with bf16():
        res = {}
        for want in ("both", "dW", "db"):
            buf = torch.full((O * K + O + 3 * PAD,), CANARY, device=DEV)
            dW, db = buf[PAD:PAD + O * K].view(O, K), buf[2 * PAD + O * K:2 * PAD + O * K + O]
            wgrad(dzd, ad, dW if want != "db" else None, db if want != "dW" else None)
            written = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
            if want != "db":
                written[PAD:PAD + O * K] = True
            if want != "dW":
                written[2 * PAD + O * K:2 * PAD + O * K + O] = True
            assert bool((buf[~written] == CANARY).all()), (want, "a float outside the requested outputs was written")
            res[want] = (dW.clone(), db.clone())
        hold(tag, "dW", res["both"][0], rW, sW, R)
        hold(tag, "db", res["both"][1], rb, sb, R)
        assert torch.equal(res["dW"][0], res["both"][0]) and torch.equal(res["db"][1], res["both"][1])
        again = torch.empty((O, K), device=DEV), torch.empty((O,), device=DEV)
        wgrad(dzd, ad, *again)
        assert torch.equal(again[0], res["both"][0]) and torch.equal(again[1], res["both"][1])


def test_nan_and_inf_stay_in_their_row():
    M, N, K = 70, 64, 48
    a, w, b, res = LR.inputs(M, N, K, 24, scaled_rows=False)
    bad = a.clone()
    bad[5, 3], bad[5, 17], bad[5, 40] = float("inf"), float("-inf"), NAN
    others = torch.arange(M) != 5
    with bf16():
        clean, dirty = TB.linear_forward(a.to(DEV), w.to(DEV), b.to(DEV)), TB.linear_forward(bad.to(DEV), w.to(DEV), b.to(DEV))
        assert torch.equal(clean[others], dirty[others]) and not bool(torch.isfinite(dirty[5]).any())
        dz, dzb = res.to(DEV), res.to(DEV).clone()
        dzb[5, 3], dzb[5, 17], dzb[5, 40] = float("inf"), float("-inf"), NAN
        clean, dirty = dgrad(dz, w.to(DEV)), dgrad(dzb, w.to(DEV))
        assert torch.equal(clean[others], dirty[others]) and not bool(torch.isfinite(dirty[5]).any())
        # an inf that survives the rounding and a value that rounds up to it
        edge = a.clone()
        edge[7, 0], edge[9, 0] = float("inf"), 3.4e38
        out = TB.linear_forward(edge.to(DEV), w.to(DEV).abs(), None)
        assert bool(torch.isinf(out[7]).all()) and bool(torch.isinf(out[9]).all()) and bool(torch.isfinite(out[8]).all())


def test_segmented_data_gradient_equals_the_packed_one():
    """dmem = dK Wk + dV Wv of the cross sublayer (the two-segment launch) against op_linear_dgrad_f32 on the packed dK | dV and torch.cat([Wk, Wv]), as
    tests/test_cross_grad_gpu.py does it in fp32 mode"""
    case = DR.make_cross_case(128, 2, TA.memory_views(2, 2, 35, 70, mask=True), 140, 280, 71, False)
    x, mem, dy, tab = case["x"].to(DEV), case["mem"].to(DEV), case["dy"].to(DEV), torch.tensor(case["views"], dtype=torch.int32)
    p = {k: v.to(DEV) for k, v in case["params"].items()}
    plist = [p[k] for k in DR.CROSS_PARAMS]
    only = tuple(n == "dmem" for n in TC.CROSS_OUTPUTS)
    with bf16():
        dmem = TC.cross_grad(x, mem, tab, *plist, dy, case["eps"], want=only)[1]
        Wk, bk, Wv, bv = (p[f"cross_attn.{n}"] for n in ("projk.weight", "projk.bias", "projv.weight", "projv.bias"))
        kv = torch.cat([TB.linear_forward(mem, Wk, bk), TB.linear_forward(mem, Wv, bv)], dim=1)
        pkv = [None if k.split(".")[1] in ("projk", "projv") else p[k] for k in DR.CROSS_PARAMS]
        dkv = TC.cross_grad(x, kv, tab, *pkv, dy, case["eps"], want=only)[1]
        packed = dgrad(dkv, torch.cat([Wk, Wv]))
        torch.cuda.synchronize()
        assert dkv.shape == (280, 256) and torch.equal(dmem, packed)
    fp32 = TC.cross_grad(x, mem, tab, *plist, dy, case["eps"], want=only)[1]
    assert not torch.equal(fp32, dmem)


def test_three_forms_run_on_the_callers_stream():
    """The harness of tests/test_stream_order_gpu.py (its delay, its bound case with the decoy inputs) on the cases op_linear_f32 and linear_grad of
    tests/stream_forms.py, unchanged, in bf16 mode: the call is queued behind a delay on a side stream while its inputs hold the decoy."""
    import stream_forms as SF
    import test_stream_order_gpu as SO
    delay = SO.Delay()
    for name in ("op_linear_f32", "linear_grad"):
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
        with TB.linear_precision("fp32"):
            assert SO.same_bits(b.reference("A"), ref_a), f"{name}: the case did not run the bf16 kernels"


# ---------------------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block_case(D, tokens, seed):
    return BR.make_case(D, D // 64, 4 * D, list(tokens), seed)


def _mlp_autograd(case, backward_in=None, forward_in=None, backward_thread=False):
    """the MLP sublayer through torch.autograd, forward and backward each inside the named precision context (None: no context)"""
    p = {k: case["params"][k].to(DEV).requires_grad_(True) for k in BR.MLP_PARAMS}
    x = case["x"].to(DEV).requires_grad_(True)
    with TB.linear_precision(forward_in):
        out = TB.mlp_sublayer(x, *[p[k] for k in BR.MLP_PARAMS], case["eps"])

    def back():
        with TB.linear_precision(backward_in):
            out.backward(case["dy"].to(DEV))
    if backward_thread:
        t = threading.Thread(target=back)
        t.start()
        t.join()
    else:
        back()
    torch.cuda.synchronize()
    return dict(out=out.detach(), dx=x.grad, **{k: t.grad for k, t in p.items()})


def _equal(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_fp32_results_do_not_depend_on_the_contexts_around_them():
    case = _block_case(128, (70,), 31)
    before = _mlp_autograd(case)
    with bf16():
        inside_bf16 = _mlp_autograd(case)
        nested = _mlp_autograd(case, forward_in="fp32", backward_in="fp32")
        assert TB.current_precision() == "bf16"
    after = _mlp_autograd(case)
    assert TB.current_precision() == "fp32"
    assert not _equal(before, nested) and not _equal(before, after)
    # the test that fails without the feature: in bf16 mode the sublayer computes something else, forward and backward
    assert len(_equal(before, inside_bf16)) == len(before), _equal(before, inside_bf16)


def test_backward_runs_in_the_precision_of_its_forward():
    case = _block_case(128, (70,), 31)
    fp32, both_inside = _mlp_autograd(case), _mlp_autograd(case, forward_in="bf16", backward_in="bf16")
    # forward inside the context, backward after it has ended (the default mode, on this thread and on another)
    assert not _equal(both_inside, _mlp_autograd(case, forward_in="bf16"))
    assert not _equal(both_inside, _mlp_autograd(case, forward_in="bf16", backward_thread=True))
    assert not _equal(both_inside, _mlp_autograd(case, forward_in="bf16", backward_in="fp32"))
    # forward in fp32, backward inside a bf16 context: the fp32 bits
    assert not _equal(fp32, _mlp_autograd(case, backward_in="bf16"))
    assert not _equal(fp32, _mlp_autograd(case, forward_in="fp32", backward_in="bf16", backward_thread=True))
    assert len(_equal(fp32, both_inside)) == len(fp32)
    # the same for the other Functions that reach a Linear: linear, the attention sublayer, the cross sublayer, the feedback offset
    g = torch.Generator().manual_seed(32)
    rn = lambda *s: torch.randn(s, generator=g).to(DEV)
    x, w, b, dy = rn(70, 128), rn(192, 128) * 0.1, rn(192), rn(70, 192)
    ccase = DR.make_cross_case(128, 2, TA.memory_views(1, 2, 35, 0, mask=True), 70, 70, 72, False)
    acase = _block_case(128, (70,), 31)
    fb = dict(x=rn(70, 128), nw=1 + 0.1 * rn(128), nb=0.1 * rn(128), w1=rn(512, 128) * 0.1, b1=0.1 * rn(512), w2=rn(128, 512) * 0.05, b2=0.1 * rn(128))

    def run(which, forward_in, backward_in):
        if which == "linear":
            leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
            with TB.linear_precision(forward_in):
                out = TB.linear(*leaves)
            up = dy
        elif which == "attn":
            leaves = [acase["x"].to(DEV).requires_grad_(True)] + [acase["params"][k].to(DEV).requires_grad_(True) for k in BR.ATTN_PARAMS]
            with TB.linear_precision(forward_in):
                out = TB.attention_sublayer(leaves[0], acase["pos"].to(DEV), acase["views"], 2, *leaves[1:], acase["rope"], acase["eps"])
            up = acase["dy"].to(DEV)
        elif which == "cross":
            leaves = [ccase["x"].to(DEV).requires_grad_(True), ccase["mem"].to(DEV).requires_grad_(True)] + \
                     [ccase["params"][k].to(DEV).requires_grad_(True) for k in DR.CROSS_PARAMS]
            with TB.linear_precision(forward_in):
                out = TC.cross_attention_sublayer(leaves[0], leaves[1], ccase["views"], 2, *leaves[2:], ccase["eps"])
            up = ccase["dy"].to(DEV)
        else:
            leaves = [t.clone().requires_grad_(True) for t in fb.values()]
            with TB.linear_precision(forward_in):
                out = TD.feedback_offset(*leaves)
            up = dy[:, :128]
        with TB.linear_precision(backward_in):
            out.backward(up)
        torch.cuda.synchronize()
        return [out.detach()] + [t.grad for t in leaves]

    for which in ("linear", "attn", "cross", "feedback"):
        inside, outside, plain, mixed = run(which, "bf16", "bf16"), run(which, "bf16", None), run(which, None, None), run(which, None, "bf16")
        assert all(torch.equal(s, t) for s, t in zip(inside, outside)), which
        assert all(torch.equal(s, t) for s, t in zip(plain, mixed)), which
        assert not torch.equal(inside[0], plain[0]) and not torch.equal(inside[1], plain[1]), which


# ---------------------------------------------------------------------------------------------------------------------------------
# the sublayers against fp64, the autocast run as the reference's own error
# ---------------------------------------------------------------------------------------------------------------------------------
_compare = functools.partial(GP.compare, _rows)


def _autocast(fn):
    with torch.autocast("cpu", dtype=torch.bfloat16):
        res = fn()
    return {k: v.float() for k, v in res.items()}


# D, tokens per view, seed: R = 19 and 70
SUB = {"d64_r19": (64, (19,), 41), "d128_r70": (128, (70,), 42)}


@functools.lru_cache(maxsize=None)
def _sub_reference(geom, which):
    case = _block_case(*SUB[geom])
    return BR.grads(case, torch.float64, which), _autocast(lambda: BR.grads(case, torch.float32, which))


@pytest.mark.parametrize("which", ["mlp", "attn"])
@pytest.mark.parametrize("geom", list(SUB))
def test_block_sublayers_match_fp64_like_autocast(geom, which):
    case = _block_case(*SUB[geom])
    g64, gac = _sub_reference(geom, which)
    names = BR.MLP_PARAMS if which == "mlp" else BR.ATTN_PARAMS
    p = [case["params"][k].to(DEV) for k in names]
    x, dy = case["x"].to(DEV), case["dy"].to(DEV)
    with bf16():
        if which == "mlp":
            out, g = TB.mlp_forward(x, *p, case["eps"]), TB.mlp_grad(x, *p, dy, case["eps"])
        else:
            pos, tab, rope = case["pos"].to(DEV), torch.tensor(case["views"], dtype=torch.int32), TB.rope_table(DEV, *case["rope"])
            out, g = TB.attn_forward(x, pos, tab, rope, *p, case["eps"]), TB.attn_grad(x, pos, tab, rope, *p, dy, case["eps"])
    torch.cuda.synchronize()
    _compare(f"{which} {geom}", dict(zip(("out", "dx") + names, [out, *g])), g64, gac)


# D, views, M, Rm, seed: memory rows that cross the 64-row key tile (19 + 70 and 70 + 70 keys per view)
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
    out.backward(case["dy"].to(DEV))
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dx=x.grad, dmem=mem.grad, **{k: t.grad for k, t in p.items()})
    assert set(got) == set(g64)
    _compare(f"cross {geom}{' key mask' if masked else ''}", got, g64, gac, mags)


# ---------------------------------------------------------------------------------------------------------------------------------
# the decoder over the branch-covering schedule
# ---------------------------------------------------------------------------------------------------------------------------------
_worst = {}


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


def _dec_run(case, dec, precision, backward_inside=True):
    dec.zero_grad(set_to_none=True)
    xs = [c["x"].to(DEV).requires_grad_(True) for c in case["calls"]]
    B, n = case["scenes"], case["n"]
    mem, loss, res = None, 0, {}
    with TB.linear_precision(precision):
        for i, (c, x) in enumerate(zip(case["calls"], xs)):
            pos = case["pos"].to(DEV).view(1, 1, n, 2).expand(B, c["V"], n, 2).contiguous()
            ts = torch.tensor([case["H"], case["W"]]).view(1, 1, 2).expand(B, c["V"], 2).contiguous()
            mem, pts, tok = dec(x, pos, ts, mem, render=c["render"], return_tokens=True)
            res[f"tokens{i}"] = tok.detach().reshape(-1, case["D"])
            loss = loss + (pts * c["G"].to(DEV)).sum()
        if backward_inside:
            loss.backward()
    if not backward_inside:
        loss.backward()
    torch.cuda.synchronize()
    res.update({f"mem{l}": m.detach() for l, m in enumerate(mem[0])})
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    res.update({k: t.grad for k, t in dec.named_parameters()})
    return res


@pytest.mark.parametrize("causal", [False, True], ids=["must3r", "causal"])
def test_decoder_matches_fp64_like_autocast_over_the_schedule(causal):
    case = _dec_case(causal)
    g64, gac, extra = _dec_reference(causal)
    dec = _dec_module(case)
    got = _dec_run(case, dec, "bf16", backward_inside=False)          # backward() after the block has ended
    names = [k for k in g64 if not k.startswith(("pointmaps", "feats"))]
    assert set(names) <= set(got)
    _compare_grouped(f"decoder {'causal' if causal else 'must3r'}", got, {k: g64[k] for k in names}, gac, dict(extra))
    inside = _dec_run(case, dec, "bf16")
    assert not [k for k in got if not torch.equal(got[k], inside[k])]
    fp32 = _dec_run(case, dec, None)
    assert not torch.equal(fp32["tokens0"], got["tokens0"]) and not torch.equal(fp32["dx0"], got["dx0"])


def test_adamw_steps_a_decoder_trained_in_bf16_mode():
    case = _dec_case(True)
    dec = _dec_module(case)
    a = _dec_run(case, dec, "bf16")
    b = _dec_run(case, dec, "bf16")
    assert not [k for k in a if not torch.equal(a[k], b[k])]
    assert all(t.grad is not None and t.grad.dtype == torch.float32 and bool(torch.isfinite(t.grad).all()) for t in dec.parameters())
    TO.AdamW(dec.parameters(), lr=1e-2).step()
    c = _dec_run(case, dec, "bf16")
    last = case["depth"] - 1
    assert not torch.equal(c["tokens0"], a["tokens0"]) and not torch.equal(c[f"mem{last}"], a[f"mem{last}"])
    assert all(t.dtype == torch.float32 for t in dec.parameters())
