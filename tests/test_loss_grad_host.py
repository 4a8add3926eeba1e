"""Host side of the loss backward (must3r_amd.train_losses; the argument checks of ``must3r_hip_metrics_loss_grad`` and
``must3r_hip_postprocess_act_grad`` through ctypes), no GPU needed: an entry point refuses bad arguments with status 1 and a message
before anything is launched, so the pointers handed over here are never followed."""
import ctypes as C

import pytest
import torch

import metrics_ref as R
from must3r_amd import _lib
from must3r_amd import losses as L
from must3r_amd import train_losses as T

RECIPE = "ConfLoss(Regr3D(L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False), alpha=0.2)"


def test_criterion_string_evaluates_in_the_module():
    crit = eval(RECIPE, vars(T))
    assert isinstance(crit, T.ConfLoss) and isinstance(crit, L.ConfLoss) and isinstance(crit.pixel_loss, T.Regr3D)
    assert crit.alpha == 0.2 and crit.pixel_loss.criterion.reduction == 'none' and crit.pixel_loss.norm_mode == 'avg_dis'
    assert not crit.pixel_loss.norm_all and T.L21.reduction == 'mean' and isinstance(T.L21, T.L21Loss)
    assert repr(crit) == repr(eval(RECIPE, vars(L)))
    for name in ("L21", "L21Loss", "Criterion", "MultiLoss", "Sum", "Regr3D", "ConfLoss", "postprocess"):
        assert hasattr(T, name), name
    assert T.Criterion is L.Criterion and T.MultiLoss is L.MultiLoss and T.Sum is L.Sum


@pytest.mark.parametrize("requires_grad", [False, True])
def test_cpu_tensors_are_refused(requires_grad):
    gt, pred = R.make_case(1, 2, 4, 5, seed=0)
    pred = {k: v.requires_grad_(requires_grad) for k, v in pred.items()}
    crit = eval(RECIPE, vars(T))
    with pytest.raises(RuntimeError, match="GPU"):
        crit(gt, pred)
    with pytest.raises(RuntimeError, match="GPU"):
        T.Regr3D(T.L21, norm_mode='avg_dis', sky_loss_value=0)(gt, pred)
    with pytest.raises(RuntimeError, match="GPU"):
        T.L21(pred['pts3d'], pred['pts3d'].detach())
    with pytest.raises(RuntimeError, match="GPU"):
        T.postprocess(torch.zeros((4, 5, 7), requires_grad=requires_grad), 'norm_exp')
    with pytest.raises(NotImplementedError, match="compute_cam"):
        T.postprocess(torch.zeros((4, 5, 7)), 'norm_exp', compute_cam=True)


class _Double:
    """A stand-in pass on the CPU: y = 2 x; ``payload`` plays the tensors a real pass keeps for its backward."""

    def __init__(self, x):
        self.payload = x.detach().clone()

    def grads(self, gos, needs):
        return (2 * gos[0],)


def test_second_order_request_raises():
    """The Function that attaches a pass to the graph is first order only, whatever the pass."""
    x = torch.arange(3.0, requires_grad=True)
    y, = T._Fused.apply(_Double(x), (2 * x.detach(),), x)
    assert y.grad_fn is not None and torch.equal(y, 2 * x.detach())
    g, = torch.autograd.grad((y * y).sum(), x, create_graph=True)      # the upstream gradient 2 y depends on x
    assert torch.equal(g.detach(), 8 * x.detach())
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        g.sum().backward()


def test_pass_is_freed_by_reference_counting_and_inplace_edits_are_noticed():
    """What a pass keeps for its backward (GBs on the device at training sizes) dies with the last reference to the loss, without the
    cyclic collector: the outputs are not reachable from the graph node.  An input modified in place before backward raises."""
    import gc
    import weakref
    x = torch.arange(3.0, requires_grad=True)
    gc.collect()
    gc.disable()
    try:
        for use in (True, False):
            run = _Double(x)
            alive = weakref.ref(run.payload)
            y, = T._Fused.apply(run, (2 * x.detach(),), x)
            del run
            if use:
                y.sum().backward()
            assert alive() is not None
            del y
            assert alive() is None
    finally:
        gc.enable()
    z = torch.arange(3.0).requires_grad_(True).clone()
    y, = T._Fused.apply(_Double(z), (2 * z.detach(),), z)
    z.mul_(2)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()


def _blocks():
    fake = C.c_void_p(0x1000)                    # never followed: every call below is refused before a launch
    a = _lib.MetricsLossArgs()
    a.n_scenes, a.n_views, a.H, a.W = 2, 3, 7, 13
    a.gt_pts = a.in_camera0 = a.pr_pts = a.valid = a.w2c = a.pr_local = a.conf = a.pr_scale = fake
    g = _lib.MetricsLossGradArgs()
    g.w_g = g.w_l = g.counts = g.grad_pts = g.grad_local = g.grad_conf = g.own_factor = g.n_valid = fake
    g.weighting, g.factor_mode, g.n_own = _lib.LOSS_W_CONF, _lib.NORM_AVG_DIS, 1
    return a, g, fake


def _refused(lib, a, g, scratch, nbytes, words):
    rc = lib.must3r_hip_metrics_loss_grad(None if a is None else C.byref(a), None if g is None else C.byref(g), scratch, nbytes, None)
    err = lib.must3r_hip_last_error().decode()
    assert rc == 1 and words in err, (rc, err, words)


def test_loss_grad_entry_point_refuses_bad_arguments():
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION >= 16
    need = lib.must3r_hip_metrics_loss_grad_scratch_bytes(2, 3, 7, 13)
    assert need > 0 and need % 256 == 0
    assert lib.must3r_hip_metrics_loss_grad_scratch_bytes(0, 3, 7, 13) == 0 and "n_scenes" in lib.must3r_hip_last_error().decode()
    a, g, fake = _blocks()
    _refused(lib, None, g, fake, need, "null argument block")
    _refused(lib, a, None, fake, need, "null argument block")
    _refused(lib, a, g, None, need, "null argument")
    _refused(lib, a, g, fake, need - 1, "scratch too small")           # everything else about these blocks is in order
    for field in ("gt_pts", "in_camera0", "pr_pts", "valid"):
        a, g, fake = _blocks()
        setattr(a, field, None)
        _refused(lib, a, g, fake, need, "null argument")
    a, g, fake = _blocks()
    a.w2c = None
    _refused(lib, a, g, fake, need, "the local term needs w2c")
    a, g, fake = _blocks()
    a.loss_in_log = 3
    _refused(lib, a, g, fake, need, "loss_in_log")
    a, g, fake = _blocks()
    a.H = 0
    _refused(lib, a, g, fake, need, "H and W must be positive")
    for bad in (-1, 4):
        a, g, fake = _blocks()
        g.weighting = bad
        _refused(lib, a, g, fake, need, "unknown weighting")
    for field, words in (("w_g", "null weight"), ("w_l", "null weight"), ("grad_pts", "grad_pts is needed"), ("grad_local", "grad_local exactly with pr_local"),
                         ("counts", "need the forward's counts"), ("grad_conf", "needs conf and grad_conf"), ("own_factor", "the scale path needs"),
                         ("n_valid", "the scale path needs")):
        a, g, fake = _blocks()
        setattr(g, field, None)
        _refused(lib, a, g, fake, need, words)
    a, g, fake = _blocks()
    a.conf = None
    _refused(lib, a, g, fake, need, "needs conf and grad_conf")
    a, g, fake = _blocks()
    a.pr_scale = None
    _refused(lib, a, g, fake, need, "the scale path needs")
    a, g, fake = _blocks()
    a.pr_local = None                            # grad_local without a local prediction
    _refused(lib, a, g, fake, need, "grad_local exactly with pr_local")
    for mode in (_lib.NORM_MEDIAN_DIS, 7):
        a, g, fake = _blocks()
        g.factor_mode = mode
        _refused(lib, a, g, fake, need, "has no scale path")
    for n_own in (-1, 3):
        a, g, fake = _blocks()
        g.n_own = n_own
        _refused(lib, a, g, fake, need, "n_own")


def test_activation_grad_entry_point_refuses_bad_arguments():
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    for args, words in (((None, _lib.ACT_NORM_EXP, fake, fake, fake, fake, 4, None), "null argument"),
                        ((fake, _lib.ACT_NORM_EXP, fake, fake, fake, None, 4, None), "null argument"),
                        ((fake, 2, fake, fake, fake, fake, 4, None), "unknown activation")):
        assert lib.must3r_hip_postprocess_act_grad(*args) == 1
        assert words in lib.must3r_hip_last_error().decode()
    assert lib.must3r_hip_postprocess_act_grad(fake, _lib.ACT_LINEAR, fake, fake, fake, fake, 0, None) == 0      # nothing to do
