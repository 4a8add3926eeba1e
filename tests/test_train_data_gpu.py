"""GPU (-m gpu): must3r_hip_gt_from_depth (csrc/train_data.hip) and must3r_amd/train_data.py against the yardstick tests/train_data_ref.py (itself held to
its fp64 form and to synthetic.SyntheticScenes by tests/test_train_data_host.py).

pts3d is held to the yardstick's bits on every pixel, the masks and n_valid exactly.  One reading of "bits": IEEE 754 leaves the sign and the payload of a NaN
that an operation produces to the implementation, and the CPU and the GPU differ there; where the yardstick has a NaN the kernel must have a NaN, every other
value must be the same 32 bits.

Shapes (B, n, Hs, Ws): (1, 1, 16, 16) 64 groups of 4 pixels, a quarter of a block; (2, 3, 32, 48) 384 groups a view, one and a half blocks, view 1 of each
scene flagged; (1, 2, 48, 80) 960 groups, no multiple of the block's 256, both flagged; (3, 1, 16, 32) the uint16 form with per-view (div, mul); and
(1, 1, 144, 256) 9216 groups = 36 blocks' worth where a view has at most 32: the walk takes a second step (flagged)."""
import ctypes as C
import functools
import time

import pytest
import torch
from torch.utils.data import DataLoader

import train_data_ref as DR
from must3r_amd import _lib, train_data as TD, train_losses as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY, BCANARY, ICANARY = -7.25e11, 0xA5, -(7 << 20)
GUARD = 64

SHAPES = {
    "1x1x16x16": dict(B=1, n=1, Hs=16, Ws=16, flagged=(), u16=False),
    "2x3x32x48": dict(B=2, n=3, Hs=32, Ws=48, flagged=(1, 4), u16=False),
    "1x2x48x80": dict(B=1, n=2, Hs=48, Ws=80, flagged=(0, 1), u16=False),
    "3x1x16x32_u16": dict(B=3, n=1, Hs=16, Ws=32, flagged=(), u16=True),
    "1x1x144x256": dict(B=1, n=1, Hs=144, Ws=256, flagged=(0,), u16=False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs on the CPU and the yardstick's outputs: computed once, shared, never modified"""
    s = SHAPES[name]
    V, Hs, Ws = s["B"] * s["n"], s["Hs"], s["Ws"]
    g = torch.Generator().manual_seed(4000 + len(name) + V * Hs)
    flags = torch.tensor([int(v in s["flagged"]) for v in range(V)], dtype=torch.int32)
    f = 0.9 * max(Hs, Ws)
    K = torch.zeros(V, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 2, 2] = f * (1 + 0.1 * torch.rand(V, generator=g)), f * (1 + 0.1 * torch.rand(V, generator=g)), 1.0
    K[:, 0, 2] = torch.where(flags != 0, Hs / 2.0, Ws / 2.0) + torch.rand(V, generator=g) - 0.5          # fractional centres: the fp64 subtraction has work
    K[:, 1, 2] = torch.where(flags != 0, Ws / 2.0, Hs / 2.0) + torch.rand(V, generator=g) - 0.5
    Q, _ = torch.linalg.qr(torch.randn(V, 3, 3, generator=g))
    pose = torch.eye(4).repeat(V, 1, 1)
    pose[:, :3, :3], pose[:, :3, 3] = Q, torch.randn(V, 3, generator=g)
    if V > 1:
        pose[V - 1] = float("nan")                      # a view without a pose
    scale = None
    if s["u16"]:
        depth = torch.randint(1, 65536, (V, Hs, Ws), generator=g, dtype=torch.int32)
        depth[torch.rand(V, Hs, Ws, generator=g) < 0.1] = 0
        depth[0, 0, :4] = torch.tensor([0, 1, 65535, 1000], dtype=torch.int32)
        depth = depth.to(torch.uint16)
        scale = torch.tensor([[1000.0, 1.0], [65535.0, 20.0], [3.0, 0.7]])[:V].contiguous()
    else:
        depth = 0.5 + 4.5 * torch.rand(V, Hs, Ws, generator=g)
        pick = torch.rand(V, Hs, Ws, generator=g)
        depth[pick < 0.1] = 0.0
        depth[pick > 0.9] = -1.0
        depth[0, 3, 5] = float("inf")
        depth[0, 0, :3] = torch.tensor([0.0, -2.0, 1.5])
    pts, valid, sky, n_valid, _ = DR.gt_from_depth(depth, K, pose, flags, scale)
    assert torch.equal(n_valid, (DR.depth_values(depth, scale) > 0).reshape(V, -1).sum(dim=1))
    if not s["u16"]:
        assert not bool(valid[0, 3, 5]) and bool(sky.any()) and bool((depth == 0).any())
    if V > 1:
        assert not bool(valid[V - 1].any()) and int(n_valid[V - 1]) > 0
    return dict(V=V, Hs=Hs, Ws=Ws, depth=depth, K=K, pose=pose, flags=flags, scale=scale, pts=pts, valid=valid, sky=sky, n_valid=n_valid)


def _dev_inputs(c):
    return {k: (None if c[k] is None else c[k].to(DEV)) for k in ("depth", "K", "pose", "flags", "scale")}


def _direct(d, V, Hs, Ws, flags=True, want=("pts3d", "valid", "sky", "n_valid"), views=None):
    """must3r_hip_gt_from_depth with every output inside an arena of canaries, GUARD elements of guard on either side; ``views``: a slice of the batch"""
    lo, hi = (0, V) if views is None else views
    n = hi - lo
    P = n * Hs * Ws
    pts = torch.full((3 * P + 2 * GUARD,), CANARY, dtype=torch.float32, device=DEV)
    valid = torch.full((P + 2 * GUARD,), BCANARY, dtype=torch.uint8, device=DEV)
    sky = torch.full((P + 2 * GUARD,), BCANARY, dtype=torch.uint8, device=DEV)
    n_valid = torch.full((n + 2 * GUARD,), ICANARY, dtype=torch.int32, device=DEV)
    scratch = torch.empty((n * _lib.GT_VIEW_BLOCKS,), dtype=torch.int32, device=DEV)
    a = _lib.GtArgs()
    a.depth = d["depth"][lo:hi].data_ptr()
    a.depth_scale = None if d["scale"] is None else d["scale"][lo:hi].data_ptr()
    a.K, a.c2w = d["K"][lo:hi].data_ptr(), d["pose"][lo:hi].data_ptr()
    a.transposed = d["flags"][lo:hi].data_ptr() if flags else None
    a.pts3d = pts.data_ptr() + 4 * GUARD if "pts3d" in want else None
    a.valid = valid.data_ptr() + GUARD if "valid" in want else None
    a.sky = sky.data_ptr() + GUARD if "sky" in want else None
    a.n_valid = n_valid.data_ptr() + 4 * GUARD if "n_valid" in want else None
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel() * 4
    a.V, a.Hs, a.Ws, a.depth_u16 = n, Hs, Ws, int(d["depth"].dtype == torch.uint16)
    a.stream = _lib.stream_ptr(torch.device(DEV))
    _lib.check(_lib.load().must3r_hip_gt_from_depth(C.byref(a)))
    torch.cuda.synchronize()
    return dict(pts3d=pts.cpu(), valid=valid.cpu(), sky=sky.cpu(), n_valid=n_valid.cpu())


def _inner(arena, name):
    return arena[name][GUARD:-GUARD]


def _guards_intact(arena, written):
    for name, canary in (("pts3d", CANARY), ("valid", BCANARY), ("sky", BCANARY), ("n_valid", ICANARY)):
        t = arena[name]
        edge = torch.cat((t[:GUARD], t[-GUARD:]))
        assert bool((edge == canary).all()), f"{name}: written outside the output"
        if name not in written:
            assert bool((t == canary).all()), f"{name}: an omitted output was written"


def _same_values(got, ref):
    """pixels whose 32 bits differ, a NaN in both counting as equal (the module docstring)"""
    gi, ri = got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)
    return int(((gi != ri) & ~(torch.isnan(got) & torch.isnan(ref))).sum())


def _check(arena, c, lo=0, hi=None, want=("pts3d", "valid", "sky", "n_valid")):
    hi = c["V"] if hi is None else hi
    if "pts3d" in want:
        bad = _same_values(_inner(arena, "pts3d").view(hi - lo, c["Hs"], c["Ws"], 3), c["pts"][lo:hi])
        print(f"pts3d: {bad} of {3 * (hi - lo) * c['Hs'] * c['Ws']} values differ from the yardstick's bits")
        assert bad == 0
    if "valid" in want:
        assert torch.equal(_inner(arena, "valid").view(hi - lo, c["Hs"], c["Ws"]), c["valid"][lo:hi].to(torch.uint8))
    if "sky" in want:
        assert torch.equal(_inner(arena, "sky").view(hi - lo, c["Hs"], c["Ws"]), c["sky"][lo:hi].to(torch.uint8))
    if "n_valid" in want:
        assert torch.equal(_inner(arena, "n_valid").to(torch.int64), c["n_valid"][lo:hi])
    _guards_intact(arena, want)


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_gives_the_yardsticks_bits_and_writes_nothing_else(name):
    c = _case(name)
    d = _dev_inputs(c)
    first = _direct(d, c["V"], c["Hs"], c["Ws"])
    _check(first, c)
    second = _direct(d, c["V"], c["Hs"], c["Ws"])
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8)), f"{k}: a second run gives other bits"


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_optional_output_omitted_in_turn(name):
    c = _case(name)
    d = _dev_inputs(c)
    every = ("pts3d", "valid", "sky", "n_valid")
    for omit in every:
        want = tuple(k for k in every if k != omit)
        _check(_direct(d, c["V"], c["Hs"], c["Ws"], want=want), c, want=want)
    _check(_direct(d, c["V"], c["Hs"], c["Ws"], want=("n_valid",)), c, want=("n_valid",))


def test_null_flag_pointer_equals_all_zero_flags():
    c = _case("2x3x32x48")
    d = _dev_inputs(c)
    null = _direct(d, c["V"], c["Hs"], c["Ws"], flags=False)
    d["flags"] = torch.zeros_like(d["flags"])
    zero = _direct(d, c["V"], c["Hs"], c["Ws"])
    flagged = _direct(_dev_inputs(c), c["V"], c["Hs"], c["Ws"])
    for k in null:
        assert torch.equal(null[k].view(torch.uint8), zero[k].view(torch.uint8)), k
    assert not torch.equal(_inner(null, "pts3d").view(torch.int32), _inner(flagged, "pts3d").view(torch.int32))
    plain = DR.gt_from_depth(c["depth"], c["K"], c["pose"])[0]
    assert _same_values(_inner(null, "pts3d").view(plain.shape), plain) == 0


@pytest.mark.parametrize("name", ["2x3x32x48", "1x2x48x80", "3x1x16x32_u16"])
def test_a_view_alone_has_the_batchs_bits(name):
    c = _case(name)
    d = _dev_inputs(c)
    whole = _direct(d, c["V"], c["Hs"], c["Ws"])
    P = c["Hs"] * c["Ws"]
    for v in range(c["V"]):
        alone = _direct(d, c["V"], c["Hs"], c["Ws"], views=(v, v + 1))
        _guards_intact(alone, ("pts3d", "valid", "sky", "n_valid"))
        assert torch.equal(_inner(alone, "pts3d").view(torch.int32), _inner(whole, "pts3d")[3 * P * v:3 * P * (v + 1)].view(torch.int32))
        for k in ("valid", "sky"):
            assert torch.equal(_inner(alone, k), _inner(whole, k)[P * v:P * (v + 1)])
        assert torch.equal(_inner(alone, "n_valid"), _inner(whole, "n_valid")[v:v + 1])


@pytest.mark.parametrize("name", ["2x3x32x48", "3x1x16x32_u16"])
def test_ground_truth_wrapper(name):
    """train_data.ground_truth: the flags from true_shape on the device, batched shapes and dtypes, the count"""
    c, s = _case(name), SHAPES[name]
    B, n, Hs, Ws = s["B"], s["n"], s["Hs"], s["Ws"]
    ts = torch.tensor([[Ws, Hs] if f else [Hs, Ws] for f in c["flags"].tolist()]).view(B, n, 2)
    G = TD.ground_truth(c["depth"].view(B, n, Hs, Ws).to(DEV), c["K"].view(B, n, 3, 3), c["pose"].view(B, n, 4, 4).to(DEV), ts.to(DEV),
                        depth_scale=None if c["scale"] is None else c["scale"].view(B, n, 2), is_metric_scale=True, count=True)
    assert G["pts3d"].shape == (B, n, Hs, Ws, 3) and G["valid_mask"].dtype == G["sky_mask"].dtype == torch.bool and G["n_valid"].shape == (B, n)
    assert _same_values(G["pts3d"].cpu().view(c["pts"].shape), c["pts"]) == 0
    assert torch.equal(G["valid_mask"].cpu().view(c["valid"].shape), c["valid"]) and torch.equal(G["sky_mask"].cpu().view(c["sky"].shape), c["sky"])
    assert torch.equal(G["n_valid"].cpu().view(-1).to(torch.int64), c["n_valid"])
    assert G["is_metric_scale"].tolist() == [True] * B and not G["is_metric_scale"].is_cuda and G["camera_pose"].is_cuda
    assert "n_valid" not in TD.ground_truth(c["depth"].view(B, n, Hs, Ws).to(DEV), c["K"].view(B, n, 3, 3), c["pose"].view(B, n, 4, 4), ts,
                                            depth_scale=None if c["scale"] is None else c["scale"].view(B, n, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# the caller's stream, and no wait on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def _stream_inputs(seed):
    ds = TD.SyntheticDepthScenes(2, 3, 32, 48, seed=seed, portrait_every=2 + seed % 2)
    batch = next(iter(DataLoader(ds, batch_size=2)))
    st = lambda k: torch.stack([b[k] for b in batch], dim=1).to(DEV)
    return dict(depth=st("depthmap"), K=st("camera_intrinsics"), pose=st("camera_pose"), ts=st("true_shape"))


def _stream_call(bufs):
    G = TD.ground_truth(bufs["depth"], bufs["K"], bufs["pose"], bufs["ts"], count=True)
    return [G["pts3d"], G["valid_mask"], G["sky_mask"], G["n_valid"]]


def test_ground_truth_runs_on_the_descriptors_stream():
    """The protocol of tests/test_encoder_grad_gpu.py::test_gather_and_patch_embed_run_on_the_descriptors_stream, with the helpers of
    tests/test_stream_order_gpu.py: reference bits of two input sets A and B on the default stream; then, with the inputs holding B, on a side stream the
    null stream overtakes: a delay, copies of A, the call, clones of the outputs, B back.  The clones must be A's bits and the delay must still be running
    when the call has returned (nothing is read back).  Control: the same call with the null stream as the stream of the descriptor and of the torch
    operations around it reproduces B's bits."""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay, null_stream
    delay = Delay()
    src = {"A": _stream_inputs(31), "B": _stream_inputs(32)}
    bufs = {k: torch.empty_like(v) for k, v in src["A"].items()}

    def load(which):
        for k, v in src[which].items():
            bufs[k].copy_(v)
    ref = {}
    for which in ("A", "A", "B"):
        load(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = _stream_call(bufs)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        ref[which] = [t.clone() for t in outs]
    assert all(not torch.equal(a, b) for a, b in zip(ref["A"], ref["B"]))
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
        outs = _stream_call(bufs)
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = [t.clone() for t in outs]
        load("B")
    s.synchronize()
    print(f"ground_truth: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the call took {side_ms:.3f} ms on the host)"
    for i, (g, r) in enumerate(zip(got, ref["A"])):
        assert torch.equal(g, r), f"output {i}: on a side stream the bits differ from the default-stream bits (equal to the decoy's: {torch.equal(g, ref['B'][i])})"
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")                         # queued behind the delay: the inputs still hold the decoy
        with torch.cuda.stream(torch.cuda.default_stream()), null_stream():
            outs = _stream_call(bufs)
            torch.cuda.default_stream().synchronize()
            got = [t.clone() for t in outs]
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    assert premise, f"the delay ({ms:.1f} ms) ended before the null stream was idle"
    for i, (g, r) in enumerate(zip(got, ref["B"])):
        assert torch.equal(g, r), f"output {i}: with the null stream the call did not run on the null stream"


# ---------------------------------------------------------------------------------------------------------------------------------
# the criterion on device-built ground truth
# ---------------------------------------------------------------------------------------------------------------------------------
def test_confloss_on_device_ground_truth_has_the_bits_of_host_built_ground_truth():
    B, n, H, W = 2, 3, 32, 48
    batch = next(iter(DataLoader(TD.SyntheticDepthScenes(B, n, H, W, seed=13, portrait_every=3), batch_size=B)))
    for b in batch:
        b["is_metric_scale"] = torch.tensor([True, False])
    imgs, ts, gt = TD.collate_views(batch, DEV)
    assert imgs.is_cuda and ts.is_cuda and all(g["pts3d"].is_cuda and set(g) == set(TD.GT_KEYS) for g in gt)
    st = lambda k: torch.stack([b[k] for b in batch], dim=1)
    pts, valid, sky, _ = DR.batched(st("depthmap"), st("camera_intrinsics"), st("camera_pose"), st("true_shape"))
    host_gt = [dict(pts3d=pts[:, i].contiguous(), valid_mask=valid[:, i].contiguous(), sky_mask=sky[:, i].contiguous(), camera_pose=b["camera_pose"],
                    is_metric_scale=b["is_metric_scale"], true_shape=b["true_shape"]) for i, b in enumerate(batch)]
    g = torch.Generator().manual_seed(14)
    noise = lambda *shape: torch.randn(shape, generator=g)
    base = dict(pts3d=torch.nan_to_num(pts) + 0.05 * noise(B, n, H, W, 3), pts3d_local=noise(B, n, H, W, 3) + torch.tensor([0.0, 0.0, 3.0]),
                conf=1.0 + torch.exp(noise(B, n, H, W)))
    crit = T.ConfLoss(T.Regr3D(T.L21, norm_mode='?avg_dis', sky_loss_value=2), alpha=0.2)
    res = {}
    for which, truth in (("device", gt), ("host", host_gt)):
        pred = {k: v.clone().to(DEV).requires_grad_(True) for k, v in base.items()}
        loss, details = crit(truth, pred)
        loss.backward()
        torch.cuda.synchronize()
        res[which] = (loss.detach().clone(), details, {k: v.grad.clone() for k, v in pred.items()})
    (la, da, ga), (lb, db, gb) = res["device"], res["host"]
    print(f"ConfLoss on device-built ground truth: loss {float(la):.6f}, details {da}")
    assert bool(torch.isfinite(la)) and torch.equal(la, lb) and da == db and set(da) == {"conf_loss_g", "conf_loss_l", "Regr3D_pts3d", "Regr3D_pts3d_local"}
    for k in ("pts3d", "pts3d_local", "conf"):
        assert bool(torch.isfinite(ga[k]).all()) and float(ga[k].abs().max()) > 0 and torch.equal(ga[k], gb[k]), k
