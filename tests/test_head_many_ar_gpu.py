"""GPU (-m gpu): the prediction head over a batch stored landscape with portrait views -- csrc/train_head.hip ``must3r_hip_head_forward_many_ar`` /
``must3r_hip_head_grad_many_ar`` through must3r_amd.train_head -- against the existing landscape-only head (bit for bit, view by view) and against the
yardstick tests/head_ar_ref.py under CPU autograd in fp64 (truth) and fp32 (the reference's own precision).

Parity is the rule of tests/grad_parity.py as tests/test_head_grad_gpu.py applies it: per case and tensor, ``e_gpu <= 4 e_ref + 32 2^-24 max|g64|``, for the five
gradients and for the forward (``out``), which is also held to that file's bound for it.  Every row is printed before it is asserted and goes, as a table, to the file
M3R_HEAD_MANY_AR_TABLE names (kept as profiles/head_many_ar_parity.txt).

Cases (V, H, W, flags, D): a lone portrait view of 6 rows; the encoder's mixed case; 143 tokens per view, so that the 128-row tiles of the backward straddle views
of different orientation, with some, all and none of the views flagged; a square batch, which is never flagged; and one case at D 128."""
import ctypes as C
import functools
import os

import pytest
import torch

import grad_parity as GP
import head_ar_ref as HAR
from must3r_amd import _lib, train_head as TH

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.25e11
PAD = 64
CASES = [(1, 32, 48, (1,), 64), (3, 48, 80, (0, 1, 0), 64), (3, 176, 208, (1, 0, 1), 64), (3, 176, 208, (1, 1, 1), 64), (3, 176, 208, (0, 0, 0), 64),
         (2, 32, 32, (0, 0), 64), (3, 48, 80, (0, 1, 0), 128)]
IDS = [f"{v}x{h}x{w}-{''.join(map(str, f))}-d{d}" for v, h, w, f, d in CASES]
PARAMS = ("gamma", "beta", "W", "b")
_rows = []

_HEADER = (
    "# tests/test_head_many_ar_gpu.py: per case (views x H x W, flags, D) and tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in",
    "# units of 2^-24 max|g64|; bound = 4 e_ref + 32; ratio = e_gpu / bound.  out: the pointmaps of the forward.  The yardstick is tests/head_ar_ref.py.",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_HEAD_MANY_AR_TABLE"), _HEADER, _rows, (34, 10), worst=True)


@functools.lru_cache(maxsize=None)
def _reference(n_views, H, Wd, flags, D):
    """(case, fp64 forward and gradients, fp32 forward and gradients): computed once, shared, never modified."""
    case = HAR.make_case(n_views, H, Wd, flags, D=D)
    r64 = dict(out=HAR.forward(case, torch.float64), **HAR.grads(case, torch.float64))
    r32 = dict(out=HAR.forward(case, torch.float32), **HAR.grads(case, torch.float32))
    return case, r64, r32


def _dev(case):
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    d["t"] = torch.tensor([int(f) for f in case["flags"]], dtype=torch.int32, device=DEV)
    return d


def _forward(d, flags="case"):
    flags = d["t"] if isinstance(flags, str) else flags
    return TH.head_forward(d["x"], d["gamma"], d["beta"], d["W"], d["b"], d["n_views"], d["H"], d["Wd"], transposed=flags)


def _grads(d, flags="case", G=None, want=(True,) * 5):
    flags = d["t"] if isinstance(flags, str) else flags
    out = TH.head_grad(d["x"], d["gamma"], d["beta"], d["W"], d["G"] if G is None else G, d["n_views"], d["H"], d["Wd"], want=want, transposed=flags)
    return dict(zip(HAR.NAMES, out))


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _guards_hold(buf, spans):
    """every float of ``buf`` outside ``spans`` [(start, stop)] still holds the canary"""
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    for lo, hi in spans:
        keep[lo:hi] = False
    return bool((buf[keep] == CANARY).all())


def _c_forward(d, flags):
    """``must3r_hip_head_forward_many_ar`` itself (``flags``: a device tensor or None for the null pointer), the output and the scratch in one canary-filled
    allocation with 64 canaries in front of, between and behind them"""
    lib = _lib.load()
    V, H, Wd, D = d["n_views"], d["H"], d["Wd"], d["D"]
    n_out = V * H * Wd * 7
    nb = lib.must3r_hip_head_forward_many_ar_scratch_bytes(V, H, Wd, D)
    assert nb % 16 == 0
    buf = torch.full((PAD + n_out + PAD + nb // 4 + PAD,), CANARY, device=DEV)
    o0, s0 = PAD, PAD + n_out + PAD
    a = _lib.HeadForwardArArgs()
    a.x, a.gamma, a.beta, a.W, a.b = (_ptr(d[k]) for k in ("x", "gamma", "beta", "W", "b"))
    a.dtype, a.n_views, a.H, a.Wimg, a.D, a.eps = _lib.F16, V, H, Wd, D, 1e-6
    a.pointmaps, a.transposed = C.c_void_p(buf.data_ptr() + 4 * o0), None if flags is None else _ptr(flags)
    a.stream = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))
    _lib.check(lib.must3r_hip_head_forward_many_ar(C.byref(a), C.c_void_p(buf.data_ptr() + 4 * s0), nb))
    torch.cuda.synchronize()
    assert _guards_hold(buf, [(o0, o0 + n_out), (s0, s0 + nb // 4)]), "a float outside the output and the scratch was written"
    out = buf[o0:o0 + n_out]
    assert bool((out != CANARY).all()), "the output was not written completely"
    return out.view(V, H, Wd, 7).clone()


def _c_grad(d, flags, want=(True,) * 5):
    """``must3r_hip_head_grad_many_ar`` itself: the five outputs and the scratch in one canary-filled allocation; an output that is not asked for is NULL"""
    lib = _lib.load()
    V, H, Wd, D = d["n_views"], d["H"], d["Wd"], d["D"]
    R = d["x"].shape[0]
    sizes = dict(dx=R * D, dgamma=D, dbeta=D, dW=HAR.HR.OUT * D, db=HAR.HR.OUT)
    nb = lib.must3r_hip_head_grad_many_ar_scratch_bytes(V, H, Wd, D)
    assert nb % 16 == 0
    off, o = {}, PAD
    for k in HAR.NAMES:
        off[k] = o
        o += sizes[k] + PAD
    s0 = o
    buf = torch.full((s0 + nb // 4 + PAD,), CANARY, device=DEV)
    a = _lib.HeadGradArArgs()
    a.g.x, a.g.gamma, a.g.beta, a.g.W, a.g.G = (_ptr(d[k]) for k in ("x", "gamma", "beta", "W", "G"))
    a.g.n_views, a.g.H, a.g.Wimg, a.g.D, a.g.eps = V, H, Wd, D, 1e-6
    for k, w in zip(HAR.NAMES, want):
        setattr(a.g, k, C.c_void_p(buf.data_ptr() + 4 * off[k]) if w else None)
    a.transposed = None if flags is None else _ptr(flags)
    a.stream = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))
    _lib.check(lib.must3r_hip_head_grad_many_ar(C.byref(a), C.c_void_p(buf.data_ptr() + 4 * s0), nb))
    torch.cuda.synchronize()
    spans = [(off[k], off[k] + sizes[k]) for k, w in zip(HAR.NAMES, want) if w]
    assert _guards_hold(buf, spans + [(s0, s0 + nb // 4)]), "a float outside the requested outputs and the scratch was written"
    got = {}
    for (lo, hi), k in zip(spans, [k for k, w in zip(HAR.NAMES, want) if w]):
        assert bool((buf[lo:hi] != CANARY).all()) and bool(torch.isfinite(buf[lo:hi]).all()), f"{k} was not written completely"
        got[k] = buf[lo:hi].clone()
    return got


def _view(d, v):
    N = d["x"].shape[0] // d["n_views"]
    return d["x"][v * N:(v + 1) * N].contiguous(), N


# ---------------------------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views,H,Wd,flags,D", CASES, ids=IDS)
def test_forward_is_the_existing_head_view_by_view(n_views, H, Wd, flags, D):
    """A flagged view is, bit for bit, the existing head on that view's tokens with the geometry (W, H), its two image axes swapped; an unflagged view is the
    existing head's.  Two runs agree; the entry point itself, between canaries, gives the same bits."""
    d = _dev(_reference(n_views, H, Wd, flags, D)[0])
    out = _forward(d)
    assert out.shape == (n_views, H, Wd, 7) and out.dtype == torch.float32
    plain = TH.head_forward(d["x"], d["gamma"], d["beta"], d["W"], d["b"], n_views, H, Wd)
    for v, f in enumerate(flags):
        if f:
            xv, _ = _view(d, v)
            want = TH.head_forward(xv, d["gamma"], d["beta"], d["W"], d["b"], 1, Wd, H)[0].swapaxes(0, 1)
            assert torch.equal(out[v], want), f"portrait view {v}"
        else:
            assert torch.equal(out[v], plain[v]), f"landscape view {v}"
    assert torch.equal(out, _forward(d))
    assert torch.equal(out, _c_forward(d, d["t"]))


@pytest.mark.parametrize("n_views,H,Wd,D", [(3, 176, 208, 64), (2, 32, 32, 64), (3, 48, 80, 128)])
def test_no_flags_give_the_existing_entry_points_bits(n_views, H, Wd, D):
    """A null flag pointer and all-zero flags: the forward and all five gradients of must3r_hip_head_forward / must3r_hip_head_grad, bit for bit"""
    d = _dev(_reference(n_views, H, Wd, (0,) * n_views, D)[0])
    zeros = torch.zeros(n_views, dtype=torch.int32, device=DEV)
    plain = TH.head_forward(d["x"], d["gamma"], d["beta"], d["W"], d["b"], n_views, H, Wd)
    assert torch.equal(_c_forward(d, None), plain) and torch.equal(_c_forward(d, zeros), plain)
    g = dict(zip(HAR.NAMES, TH.head_grad(d["x"], d["gamma"], d["beta"], d["W"], d["G"], n_views, H, Wd)))
    for got in (_c_grad(d, None), _c_grad(d, zeros)):
        for k in HAR.NAMES:
            assert torch.equal(got[k], g[k].reshape(-1)), k


def test_any_non_zero_flag_means_portrait():
    d = _dev(_reference(3, 176, 208, (1, 0, 1), 64)[0])
    odd = torch.tensor([5, 0, -1], dtype=torch.int32, device=DEV)
    big = torch.tensor([1 << 30, 0, -(1 << 31)], dtype=torch.int32, device=DEV)
    out, g = _forward(d), _grads(d)
    for flags in (odd, big):
        assert torch.equal(_forward(d, flags), out)
        got = _grads(d, flags)
        for k in HAR.NAMES:
            assert torch.equal(got[k], g[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# the backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views,H,Wd,flags,D", CASES, ids=IDS)
def test_dx_of_each_view_is_the_composed_form_on_that_view_alone(n_views, H, Wd, flags, D):
    """Under autograd: the existing landscape-only head on the view's tokens, with ``swapaxes`` for a portrait view, fed the view's part of the upstream
    gradient.  The rows of dx of the batch call are its bits, whatever the orientation of the views that share a 128-row tile with them."""
    d = _dev(_reference(n_views, H, Wd, flags, D)[0])
    dx = _grads(d, want=(True, False, False, False, False))["dx"]
    for v, f in enumerate(flags):
        xv, N = _view(d, v)
        xv = xv.clone().requires_grad_(True)
        params = (d["gamma"], d["beta"], d["W"], d["b"])
        if f:
            out = TH.prediction_head(xv.view(1, N, D), (Wd, H), *params).swapaxes(1, 2)
        else:
            out = TH.prediction_head(xv.view(1, N, D), (H, Wd), *params)
        out.backward(d["G"][v:v + 1])
        assert torch.equal(dx[v * N:(v + 1) * N], xv.grad), f"view {v} (portrait: {bool(f)})"


@pytest.mark.parametrize("n_views,H,Wd,flags,D", CASES, ids=IDS)
def test_forward_and_gradients_match_fp64(n_views, H, Wd, flags, D):
    """The forward and the gradients by the parity rule; the forward, which is the existing head's split-precision forward, also by the bound
    tests/test_head_grad_gpu.py holds that one to (rtol 1e-5, atol 1e-4 against fp64)."""
    case, r64, r32 = _reference(n_views, H, Wd, flags, D)
    d = _dev(case)
    tag = f"{n_views}x{H}x{Wd} {''.join(map(str, flags))} D{D}"
    out = _forward(d)
    assert torch.allclose(out.cpu().double(), r64["out"], rtol=1e-5, atol=1e-4), float((out.cpu().double() - r64["out"]).abs().max())
    GP.compare(_rows, tag, dict(out=out, **_grads(d)), r64, r32)


def test_autograd_through_prediction_head():
    """``prediction_head(..., transposed=flags)`` under autograd: the five gradients are the entry point's bits, and the flags are not differentiated"""
    n_views, H, Wd, flags, D = 3, 48, 80, (0, 1, 0), 64
    d = _dev(_reference(n_views, H, Wd, flags, D)[0])
    leaves = [d[k].clone().requires_grad_(True) for k in ("x", *PARAMS)]
    out = TH.prediction_head(leaves[0].view(n_views, -1, D), (H, Wd), *leaves[1:], transposed=d["t"])
    assert torch.equal(out, _forward(d))
    out.backward(d["G"])
    g = _grads(d)
    for k, leaf in zip(HAR.NAMES, leaves):
        assert torch.equal(leaf.grad, g[k]), k
    with torch.no_grad():
        assert torch.equal(TH.prediction_head(d["x"].view(n_views, -1, D), (H, Wd), *(d[k] for k in PARAMS), transposed=d["t"]), out)


def test_module_computes_the_flags_on_the_device():
    """``PredictionHead(landscape_only=True)``: with img_shape and without it (H, W from the host's min / max) the bits of the operator with the flags given"""
    n_views, H, Wd, flags, D = 3, 48, 80, (0, 1, 0), 64
    d = _dev(_reference(n_views, H, Wd, flags, D)[0])
    head = TH.PredictionHead(D, landscape_only=True)
    with torch.no_grad():
        for p, k in zip(head.parameters(), PARAMS):
            p.copy_(d[k])
    head = head.to(DEV)
    ts = HAR.true_shape(flags, H, Wd)
    want = _forward(d)
    tok = d["x"].view(1, n_views, -1, D)
    with torch.no_grad():
        for shape in (ts.view(1, n_views, 2), ts.to(DEV).view(1, n_views, 2)):
            assert torch.equal(head(tok, shape)[0], want)
            assert torch.equal(head(tok, shape, img_shape=(H, Wd))[0], want)
    with pytest.raises(ValueError, match="share"):
        TH.PredictionHead(D).to(DEV)(tok, ts)


def test_backward_repeats_bitwise():
    d = _dev(_reference(3, 176, 208, (1, 0, 1), 64)[0])
    a, b = _grads(d), _grads(d)
    for k in HAR.NAMES:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("want", [(True, False, False, False, False), (False, False, False, True, True), (True, True, True, False, False),
                                  (False, False, False, False, True), (False, False, False, True, False), (True, True, True, True, True)], ids=str)
def test_every_gradient_is_optional_and_canaries_survive(want):
    """429 rows with views of both orientations: the five outputs and the scratch lie in one canary-filled allocation; an output that is not asked for is
    NULL, and every float outside the requested outputs and the scratch keeps its canary.  A requested output has the bits of the full call."""
    d = _dev(_reference(3, 176, 208, (1, 0, 1), 64)[0])
    full = _grads(d)
    got = _c_grad(d, d["t"], want)
    assert set(got) == {k for k, w in zip(HAR.NAMES, want) if w}
    for k, t in got.items():
        assert torch.equal(t, full[k].reshape(-1)), k


def test_nan_upstream_pixel_of_a_portrait_view_stays_in_its_row():
    """Stored pixel (y, x) of a portrait view belongs to the token (py, px) = (x // 16, y // 16) of its grid of W/16 rows of H/16 columns"""
    n_views, H, Wd = 3, 176, 208
    d = _dev(_reference(n_views, H, Wd, (1, 0, 1), 64)[0])
    G = d["G"].clone()
    v, y, x = 2, 37, 101
    G[v, y, x, 4] = float("nan")
    row = v * (H // 16) * (Wd // 16) + (x // 16) * (H // 16) + y // 16
    dx = _grads(d, G=G, want=(True, False, False, False, False))["dx"]
    assert torch.isnan(dx).any(dim=1).nonzero().flatten().tolist() == [row]
