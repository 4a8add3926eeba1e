"""GPU (-m gpu): the prediction head's training forward and backward -- csrc/train_head.hip ``must3r_hip_head_forward`` /
``must3r_hip_head_grad`` and the operator-level entry points, through must3r_amd.train_head -- against the yardstick tests/head_ref.py
under CPU autograd, fed the same fp32 inputs in fp64 (truth) and in fp32 (the reference's own precision).

Gradient parity is the rule of tests/test_loss_grad_gpu.py, unchanged: per case and tensor, ``e_gpu`` = max |GPU - fp64|, ``e_ref`` = max |fp32 CPU
autograd - fp64|, required ``e_gpu <= 4 e_ref + 32 2^-24 max|g64|``.  Every row is printed before it is asserted and goes, as a table, to the file
M3R_HEAD_GRAD_TABLE names (kept as profiles/head_grad_parity.txt).  The upstream gradient is of order 1e-7, below fp16's range.

The exact conditions (determinism, independence of a view from its batch, zero and NaN upstream gradients, linearity, outputs that were not
asked for, canaries) have no tolerance.
"""
import ctypes as C
import functools
import os

import pytest
import torch

import grad_parity as GP
import head_ref as HR
import metrics_ref as MR
from must3r_amd import _lib, train_head as TH, train_losses as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(1, 32, 48), (3, 48, 32), (3, 176, 208), (2, 160, 512)]
CANARY = -7.25e11
_rows = []

_HEADER = (
    "# tests/test_head_grad_gpu.py: per case and gradient tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in",
    "# units of 2^-24 max|g64|; bound = 4 e_ref + 32; ratio = e_gpu / bound.  Every tensor is held to this bound (no componentwise bound was needed).",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_HEAD_GRAD_TABLE"), _HEADER, _rows, (34, 10), worst=False)


@functools.lru_cache(maxsize=None)
def _reference(n_views, H, Wd):
    """(case, forward in fp64, gradients in fp64, gradients in fp32): computed once, shared, never modified."""
    case = HR.make_case(n_views, H, Wd)
    return case, HR.forward(case, torch.float64), HR.grads(case, torch.float64), HR.grads(case, torch.float32)


def _dev(case):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def _gpu_grads(d, G=None, want=(True,) * 5):
    out = TH.head_grad(d["x"], d["gamma"], d["beta"], d["W"], d["G"] if G is None else G, d["n_views"], d["H"], d["Wd"], want=want)
    torch.cuda.synchronize()
    return dict(zip(HR.NAMES, out))


_compare = functools.partial(GP.compare, _rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views,H,Wd", CASES)
def test_gradients_match_autograd(n_views, H, Wd):
    """(1,32,48): 6 rows, all tail; (3,48,32): portrait grid, view indexing of the gather; (3,176,208): 429 rows, full tiles plus a tail and four
    splits of the weight gradient; (2,160,512): 640 rows, the model's widest grid."""
    case, _, g64, g32 = _reference(n_views, H, Wd)
    _compare(f"head {n_views}x{H}x{Wd}", _gpu_grads(_dev(case)), g64, g32)


@pytest.mark.parametrize("n_views,H,Wd", CASES)
def test_forward_matches_fp64_and_repeats(n_views, H, Wd):
    case, f64, _, _ = _reference(n_views, H, Wd)
    d = _dev(case)
    outs = [TH.prediction_head(d["x"].view(n_views, -1, d["D"]), (H, Wd), d["gamma"], d["beta"], d["W"], d["b"]) for _ in range(2)]
    assert outs[0].shape == (n_views, H, Wd, 7) and outs[0].dtype == torch.float32
    err = float((outs[0].cpu().double() - f64).abs().max())
    print(f"forward {n_views}x{H}x{Wd}: max abs error {err:.3e} of max|out| {float(f64.abs().max()):.3e}")
    assert torch.allclose(outs[0].cpu().double(), f64, rtol=1e-5, atol=1e-4), err
    assert torch.equal(outs[0], outs[1])


def test_operator_entry_points_width_128():
    """D = 128 through the plain operand forms (a hard-coded 768 would show): dZ with a leading dimension, 150 rows = one tile and a tail,
    two splits of the weight gradient."""
    lib = _lib.load()
    M, O, K, ldz = 150, 1792, 128, 1800
    g = torch.Generator().manual_seed(5)
    dZ_full = torch.randn((M, ldz), generator=g) * 1e-7
    dZ = dZ_full[:, :O]
    W = (torch.rand((O, K), generator=g) * 2 - 1) * 0.05
    x = torch.randn((M, K), generator=g) * (0.5 + torch.rand((M, 1), generator=g)) + torch.randn((M, 1), generator=g)
    gamma = 1.0 + 0.2 * torch.randn((K,), generator=g)
    dy = torch.randn((M, K), generator=g) * 1e-7
    stream = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    dZ_d, W_d, x_d, gamma_d, dy_d = (t.to(DEV).contiguous() for t in (dZ_full, W, x, gamma, dy))
    # data gradient
    out = torch.full((M, K), CANARY, device=DEV)
    _lib.check(lib.must3r_hip_op_linear_dgrad_f32(ptr(dZ_d), ldz, ptr(W_d), ptr(out), M, O, K, stream))
    # weight gradient
    assert TH.wgrad_splits(M) == 2
    nb = lib.must3r_hip_op_linear_wgrad_scratch_bytes(M, O, K)
    scratch = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    dW, db = torch.full((O, K), CANARY, device=DEV), torch.full((O,), CANARY, device=DEV)
    _lib.check(lib.must3r_hip_op_linear_wgrad_f32(ptr(dZ_d), ldz, ptr(x_d), K, ptr(dW), ptr(db), M, O, K, ptr(scratch), nb, stream))
    # LayerNorm backward
    nb2 = lib.must3r_hip_op_layernorm_grad_scratch_bytes(M, K)
    scratch2 = torch.empty((nb2,), dtype=torch.uint8, device=DEV)
    dx, dg, dbeta = torch.full((M, K), CANARY, device=DEV), torch.full((K,), CANARY, device=DEV), torch.full((K,), CANARY, device=DEV)
    _lib.check(lib.must3r_hip_op_layernorm_grad(ptr(x_d), ptr(gamma_d), ptr(dy_d), ptr(dx), ptr(dg), ptr(dbeta), M, K, 1e-6, ptr(scratch2), nb2, stream))
    torch.cuda.synchronize()

    def ref(dt):
        z, w, a = dZ.to(dt), W.to(dt), x.to(dt)
        xl, gl, bl = a.clone().requires_grad_(True), gamma.to(dt).clone().requires_grad_(True), torch.zeros(K, dtype=dt, requires_grad=True)
        torch.nn.functional.layer_norm(xl, (K,), gl, bl, 1e-6).backward(dy.to(dt))
        return dict(dgrad=z @ w, wgrad=z.t() @ a, bsum=z.sum(0), ln_dx=xl.grad, ln_dgamma=gl.grad, ln_dbeta=bl.grad)
    _compare("ops D=128 M=150", dict(dgrad=out, wgrad=dW, bsum=db, ln_dx=dx, ln_dgamma=dg, ln_dbeta=dbeta), ref(torch.float64), ref(torch.float32))


def test_forward_linear_stage_equals_decoder_bits():
    """The native decoder and the training forward share the head's launches: the decoder's own post-LayerNorm tensor (``return_feats``) through
    the Linear stage, on the head's fp32 copies of the decoder's parameters, gives the decoder's pointmaps of that same call bit for bit."""
    from must3r_amd import synthetic as S
    from must3r_amd.config import TINY
    from test_model_gpu import build
    enc, dec = build(TINY, "fp16w2")
    imgs, ts = S.make_images(2, 48, 64, 4)
    x, pos = enc(imgs.cuda(), ts.cuda())
    _, pm, feats = dec(x.unsqueeze(0), pos.unsqueeze(0), ts.cuda().unsqueeze(0), None, return_feats=True)
    head = TH.PredictionHead.from_decoder(dec)
    assert list(head.state_dict()) == ["norm_dec.weight", "norm_dec.bias", "head_dec.proj.weight", "head_dec.proj.bias"]
    y = feats[-1].reshape(-1, TINY.dec_dim)
    again = TH.head_linear(y, head.head_dec.proj.weight, head.head_dec.proj.bias, 2, 48, 64)
    torch.cuda.synchronize()
    assert torch.equal(again.view_as(pm), pm)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact conditions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_backward_repeats_bitwise():
    d = _dev(_reference(3, 176, 208)[0])
    a, b = _gpu_grads(d), _gpu_grads(d)
    for k in HR.NAMES:
        assert torch.equal(a[k], b[k]), k


def test_view_alone_equals_view_in_batch():
    d = _dev(_reference(3, 48, 32)[0])
    N = (48 // 16) * (32 // 16)
    full = _gpu_grads(d, want=(True, False, False, False, False))["dx"]
    for v in range(3):
        one = TH.head_grad(d["x"][v * N:(v + 1) * N].contiguous(), d["gamma"], d["beta"], d["W"], d["G"][v:v + 1].contiguous(), 1, 48, 32,
                           want=(True, False, False, False, False))[0]
        assert torch.equal(one, full[v * N:(v + 1) * N]), v


def test_zero_upstream_view_gives_zero_rows():
    d = _dev(_reference(3, 48, 32)[0])
    N = 6
    full = _gpu_grads(d)["dx"]
    G = d["G"].clone()
    G[1] = 0
    got = _gpu_grads(d, G=G)["dx"]
    assert bool((got[N:2 * N] == 0).all())
    assert torch.equal(got[:N], full[:N]) and torch.equal(got[2 * N:], full[2 * N:])


def test_backward_is_linear_in_the_upstream_gradient():
    d = _dev(_reference(3, 176, 208)[0])
    a, b = _gpu_grads(d), _gpu_grads(d, G=d["G"] * 2)
    for k in HR.NAMES:
        assert torch.equal(a[k] * 2, b[k]), k


def test_nan_upstream_pixel_stays_in_its_row():
    n_views, H, Wd = 3, 176, 208
    d = _dev(_reference(n_views, H, Wd)[0])
    G = d["G"].clone()
    v, py, px = 1, 37, 101
    G[v, py, px, 4] = float("nan")
    row = v * (H // 16) * (Wd // 16) + (py // 16) * (Wd // 16) + px // 16
    dx = _gpu_grads(d, G=G, want=(True, False, False, False, False))["dx"]
    nan_rows = torch.isnan(dx).any(dim=1)
    assert bool(torch.isnan(dx[row]).all())
    assert nan_rows.nonzero().flatten().tolist() == [row]


@pytest.mark.parametrize("want", [(True, False, False, False, False), (False, False, False, True, True), (True, True, True, False, False),
                                  (False, False, False, False, True), (True, True, True, True, True)], ids=str)
def test_unrequested_outputs_and_canaries(want):
    """The five outputs lie in one canary-filled allocation with 64 canaries in front of, between and behind them; an output that is not asked
    for is passed as NULL.  Its floats, and every canary, must survive; a requested output is written completely (429 rows: tail rows too)."""
    lib = _lib.load()
    n_views, H, Wd = 3, 176, 208
    case, _, g64, _ = _reference(n_views, H, Wd)
    d = _dev(case)
    R, D, PAD = d["x"].shape[0], d["D"], 64
    sizes = dict(dx=R * D, dgamma=D, dbeta=D, dW=HR.OUT * D, db=HR.OUT)
    buf = torch.full((sum(sizes.values()) + PAD * (len(sizes) + 1),), CANARY, device=DEV)
    off, o = {}, PAD
    for k in HR.NAMES:
        off[k] = o
        o += sizes[k] + PAD
    a = _lib.HeadGradArgs()
    a.x, a.gamma, a.beta, a.W, a.G = (C.c_void_p(d[k].data_ptr()) for k in ("x", "gamma", "beta", "W", "G"))
    a.n_views, a.H, a.Wimg, a.D, a.eps = n_views, H, Wd, D, 1e-6
    for k, w in zip(HR.NAMES, want):
        setattr(a, k, C.c_void_p(buf.data_ptr() + 4 * off[k]) if w else None)
    nb = lib.must3r_hip_head_grad_scratch_bytes(n_views, H, Wd, D)
    scratch = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    _lib.check(lib.must3r_hip_head_grad(C.byref(a), C.c_void_p(scratch.data_ptr()), nb, C.c_void_p(_lib.stream_ptr(torch.device(DEV)))))
    torch.cuda.synchronize()
    written = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    for k, w in zip(HR.NAMES, want):
        if w:
            written[off[k]:off[k] + sizes[k]] = True
    assert bool((buf[~written] == CANARY).all()), "a float outside the requested outputs was written"
    assert bool((buf[written] != CANARY).all()) and bool(torch.isfinite(buf[written]).all()), "a requested output was not written completely"
    full = _gpu_grads(d)
    for k, w in zip(HR.NAMES, want):
        if w:
            assert torch.equal(buf[off[k]:off[k] + sizes[k]].view_as(full[k]), full[k]), k


def test_entry_point_refusals():
    lib = _lib.load()
    d = _dev(_reference(1, 32, 48)[0])
    dx = torch.empty_like(d["x"])
    nb = lib.must3r_hip_head_grad_scratch_bytes(1, 32, 48, 768)
    scratch = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))

    def call(nbytes=nb, **over):
        a = _lib.HeadGradArgs()
        a.x, a.gamma, a.beta, a.W, a.G = (C.c_void_p(d[k].data_ptr()) for k in ("x", "gamma", "beta", "W", "G"))
        a.n_views, a.H, a.Wimg, a.D, a.eps = 1, 32, 48, 768, 1e-6
        a.dx = C.c_void_p(dx.data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        return lib.must3r_hip_head_grad(C.byref(a), C.c_void_p(scratch.data_ptr()), nbytes, stream)
    assert call() == 0
    for over, word in ((dict(G=None), "null"), (dict(x=None), "null"), (dict(H=40), "multiples of 16"), (dict(Wimg=50), "multiples of 16"),
                       (dict(D=96), "multiple of 64"), (dict(nbytes=nb - 1), "scratch")):
        assert call(**over) != 0, over
        assert word in lib.must3r_hip_last_error().decode(), (over, lib.must3r_hip_last_error())
    assert lib.must3r_hip_head_grad_scratch_bytes(1, 40, 48, 768) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_training_chain_end_to_end():
    """tokens -> PredictionHead -> train_losses.postprocess -> ConfLoss(Regr3D(L21, '?avg_dis', sky 2), alpha 0.2) -> backward, 2 scenes x 2 views of
    32 x 48, against head_ref composed with metrics_ref under fp64 autograd (same rule); then one SGD step on the head, which must move all
    four parameters and lower the fp64 loss.  The step length comes from the fp64 gradient: 0.05 in parameter space."""
    B, V, H, Wd, D = 2, 2, 32, 48, 768
    gt, _ = MR.make_case(B, V, H, Wd, 3, scale=2.0, sky_frac=0.1, metric=[True, False])
    case = HR.make_case(B * V, H, Wd, seed=3)
    keys = ("x", "gamma", "beta", "W", "b")

    def yardstick(dt, params=None):
        leaves = [(case[k] if params is None else params[k]).to(dt).clone().requires_grad_(True) for k in keys]
        raw = HR.head(*leaves, B * V, H, Wd).view(B, V, H, Wd, 7)
        crit = MR.ConfLoss(MR.Regr3D(MR.L21, norm_mode='?avg_dis', sky_loss_value=2), alpha=0.2)
        loss, _ = crit(MR.to64(gt) if dt == torch.float64 else gt, HR.postprocess(raw))
        loss.backward()
        return float(loss), {n: t.grad for n, t in zip(HR.NAMES, leaves)}
    loss64, g64 = yardstick(torch.float64)
    _, g32 = yardstick(torch.float32)

    head = TH.PredictionHead(D)
    with torch.no_grad():
        for p, k in zip(head.parameters(), keys[1:]):
            p.copy_(case[k])
    head = head.to(DEV)
    tokens = case["x"].view(B, V, -1, D).to(DEV).requires_grad_(True)
    true_shape = torch.tensor([[[H, Wd]] * V] * B)
    gt_d = [{k: v.to(DEV) for k, v in b.items()} for b in gt]
    crit = T.ConfLoss(T.Regr3D(T.L21, norm_mode='?avg_dis', sky_loss_value=2), alpha=0.2)
    raw = head(tokens, true_shape)
    assert raw.shape == (B, V, H, Wd, 7)
    loss, _ = crit(gt_d, T.postprocess(raw, 'norm_exp'))
    loss.backward()
    print(f"end to end: loss {float(loss):.6f} (fp64 yardstick {loss64:.6f})")
    params = list(head.parameters())
    got = dict(dx=tokens.grad.reshape(-1, D), dgamma=params[0].grad, dbeta=params[1].grad, dW=params[2].grad, db=params[3].grad)
    _compare("end to end 2x2x32x48", got, g64, g32)

    before = [p.detach().clone() for p in params]
    norm = float(sum((g64[n] ** 2).sum() for n in HR.NAMES[1:]).sqrt())
    torch.optim.SGD(head.parameters(), lr=0.05 / norm).step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, params))
    stepped = dict(x=case["x"], **{k: p.detach().cpu() for k, p in zip(keys[1:], params)})
    loss_after, _ = yardstick(torch.float64, stepped)
    print(f"end to end: fp64 loss {loss64:.6f} -> {loss_after:.6f} after one SGD step of length 0.05")
    assert loss_after < loss64
