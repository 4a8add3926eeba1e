"""GPU (-m gpu): the scene renderer (must3r_amd.render / csrc/render.hip) against the numpy restatement tests/render_ref.py, bit for bit: colour,
depth and source index of every target pixel.  Nothing here reads the reference checkout."""
import os
import time

import numpy as np
import pytest
import torch

import export_ref as R
import render_ref as RR
from must3r_amd import demo as Dm, render as Rn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIXED = [(48, 64), (48, 64), (32, 64), (32, 64), (48, 64)]
RAGGED = [(7, 13), (33, 37), (1, 5), (40, 64)]
EMPTY = 0xFFFFFFFF
_cache = {}


def _scene(shapes=MIXED, seed=0):
    key = ("scene", tuple(shapes), seed)
    if key not in _cache:
        scene = R.make_scene(shapes, seed=seed)
        _cache[key] = (scene, R.scene_views(scene, False), R.scene_views(scene, True))
    return _cache[key]


def _cam(scene, i, f=40.0, W=64, H=48, cx=None, cy=None):
    c = RR.pose_camera(scene.cams2world[i], f, W, H)
    return c if cx is None else c._replace(cx=cx, cy=cy)


def _want(name, views, matrices, cam, thr, ps=1, bg=(255, 255, 255)):
    """the restatement's images, computed once per named case and left unchanged"""
    key = ("want", name, ps, bg, float(thr))
    if key not in _cache:
        _cache[key] = RR.render(views, matrices, cam, thr, ps, bg)
    return _cache[key]


def _np(images):
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in im.items()} for im in images]


def _render(views, matrices, cams, thr, ps=1, bg=(255, 255, 255), want=("rgb", "depth", "index"), **kw):
    M = None if matrices is None else np.stack([np.asarray(m, dtype=np.float64) for m in matrices])
    return _np(Rn.SceneRenderer(views, M, device=DEV, **kw).render(cams, thr, ps, bg, want))


def _equal(got, want, what=""):
    rgb, depth, index = want
    assert got["index"].dtype == np.uint32 and got["depth"].dtype == np.float32 and got["rgb"].dtype == np.uint8
    assert np.array_equal(got["index"], index), what
    assert np.array_equal(got["depth"].view(np.uint32), depth.view(np.uint32)), what
    assert np.array_equal(got["rgb"], rgb), what


# ---------------------------------------------------------------------------------------------------------------------------------
# the main case
# ---------------------------------------------------------------------------------------------------------------------------------
def test_main_case_equals_restatement():
    scene, views, _ = _scene()
    cams = [_cam(scene, 0), _cam(scene, 1)]
    M = RR.identity(len(views))
    # the inputs first, on the CPU: a trivial image cannot pass these
    for cam in cams:
        pix, _, st = RR.contenders(views, M, cam, 1.5)
        cnt = np.bincount(pix, minlength=64 * 48)
        covered, multi = float((cnt > 0).mean()), float((cnt >= 2).mean())
        print(f"covered {covered:.3f}, two or more contenders {multi:.3f}, behind {st['behind']}, outside {st['outside']} of {st['selected']} selected")
        assert 0.3 <= covered <= 0.7 and multi >= 0.15 and st["behind"] >= 1000 and st["outside"] >= 1000
    got = _render(views, None, cams, 1.5)
    for i, cam in enumerate(cams):
        _equal(got[i], _want(f"main{i}", views, M, cam, 1.5), f"camera {i}")
    assert got[0]["rgb"].shape == (48, 64, 3) and got[0]["depth"].shape == (48, 64) and got[0]["index"].shape == (48, 64)


# ---------------------------------------------------------------------------------------------------------------------------------
# further cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,f,ps", [(1, 1, 1e-3, 1), (5, 3, 2.0, 1), (67, 45, 25.0, 2)])
def test_target_sizes(W, H, f, ps):
    scene, views, _ = _scene()
    cam = _cam(scene, 0, f, W, H)
    M = RR.identity(len(views))
    pix, _, st = RR.contenders(views, M, cam, 1.5, ps)
    if (W, H) == (1, 1):
        # every selected point in front of the camera contends for the one pixel
        assert len(pix) == st["selected"] - st["behind"] > 4000
    else:
        assert np.bincount(pix, minlength=W * H).min() >= 0 and len(np.unique(pix)) > W * H // 3
    got = _render(views, None, [cam], 1.5, ps)[0]
    _equal(got, _want(f"size{W}x{H}", views, M, cam, 1.5, ps))
    assert got["index"].shape == (H, W)


@pytest.mark.parametrize("ps", [1, 2, 3, 8])
def test_point_sizes_straddle_every_edge(ps):
    scene, views, _ = _scene()
    cam = _cam(scene, 1)
    M = RR.identity(len(views))
    if ps > 1:
        # squares that are cut by each of the four edges exist among the kept points
        left = right = top = bottom = 0
        for (conf, pts, _), m in zip(views, M):
            Z, u, v = RR.project(RR.compose(cam.w2c, m), cam, pts.reshape(-1, 3))
            ok = R.select(conf.reshape(-1), 1.5) & (Z >= 0.01) & (Z <= 100)
            c0, r0 = np.floor(u - 0.5 * (ps - 1)), np.floor(v - 0.5 * (ps - 1))
            inr, inc = (r0 >= 0) & (r0 + ps <= 48), (c0 >= 0) & (c0 + ps <= 64)
            left += int((ok & inr & (c0 < 0) & (c0 + ps > 0)).sum())
            right += int((ok & inr & (c0 < 64) & (c0 + ps > 64)).sum())
            top += int((ok & inc & (r0 < 0) & (r0 + ps > 0)).sum())
            bottom += int((ok & inc & (r0 < 48) & (r0 + ps > 48)).sum())
        assert min(left, right, top, bottom) >= 3, (left, right, top, bottom)
    _equal(_render(views, None, [cam], 1.5, ps)[0], _want("ps", views, M, cam, 1.5, ps))


def test_ragged_views():
    scene, views, _ = _scene(RAGGED, 0)
    M = RR.identity(len(views))
    cams = [_cam(scene, 1, 20.0, 37, 33), _cam(scene, 3)]
    assert len({(c.W, c.H) for c in cams}) == 2          # two sizes in one render(): grouped
    got = _render(views, None, cams, 1.5, 2)
    for i, cam in enumerate(cams):
        want = _want(f"ragged{i}", views, M, cam, 1.5, 2)
        assert len(np.unique(want[2])) > 100
        _equal(got[i], want, i)
    # every view shows up somewhere, the 5-pixel one included, when everything is selected
    want = _want("ragged_all", views, M, _cam(scene, 1, 2.0, 16, 16), 0.0, 1)
    bases = np.cumsum([0] + [h * w for h, w in RAGGED])
    seen = want[2][want[2] != EMPTY]
    assert all(((seen >= bases[i]) & (seen < bases[i + 1])).any() for i in range(4))
    _equal(_render(views, None, [_cam(scene, 1, 2.0, 16, 16)], 0.0, 1)[0], want)


def test_many_small_views_and_camera_groups():
    """130 views of 5 pixels (one source block each) and 127 cameras: the launch walks 8 cameras per block, the last group holds 7"""
    shapes = [(1, 5)] * 130
    scene, views, _ = _scene(shapes, 5)
    M = RR.identity(len(views))
    cams = [_cam(scene, i, 3.0, 5, 3) for i in range(127)]
    got = _render(views, None, cams, 1.2)
    hits = 0
    for i in (0, 7, 8, 63, 119, 120, 126):
        want = RR.render(views, M, cams[i], 1.2)
        hits += int((want[2] != EMPTY).sum())
        _equal(got[i], want, i)
    assert hits > 30


def test_local_pointmaps_with_camera_matrices():
    scene, _, views_local = _scene()
    M = [R.np64(c)[:3] for c in scene.cams2world]
    for i in (0, 1):
        cam = _cam(scene, i)
        want = _want(f"local{i}", views_local, M, cam, 1.5)
        assert 0.3 < float((want[2] != EMPTY).mean()) < 0.7
        _equal(_render(views_local, M, [cam], 1.5)[0], want)


def test_planted_tie_goes_to_the_lower_index():
    scene, views, _ = _scene()
    views = [tuple(a.copy() for a in v) for v in views]
    n3 = 32 * 64
    base1, base3 = 48 * 64, 48 * 64 * 2 + 32 * 64
    # view 3's points (and confidences) over the first 32 rows of view 1: every point of view 3 has a twin of equal depth and lower index
    views[1][1].reshape(-1, 3)[:n3] = views[3][1].reshape(-1, 3)
    views[1][0].reshape(-1)[:n3] = views[3][0].reshape(-1)
    M = RR.identity(len(views))
    cam = _cam(scene, 3)                  # view 3's own pose: its points fill the image
    before = _want("pose3", _scene()[1], M, cam, 1.5)[2]
    assert ((before >= base3) & (before < base3 + n3)).sum() > 50
    want = RR.render(views, M, cam, 1.5)
    twins = (want[2] >= base1) & (want[2] < base1 + n3)
    assert not ((want[2] >= base3) & (want[2] < base3 + n3)).any() and twins.sum() > 50
    _equal(_render(views, None, [cam], 1.5)[0], want)


def test_nan_and_inf_in_points_and_confidences():
    scene, views, _ = _scene([(33, 37), (48, 64)], 2)
    views = [tuple(a.copy() for a in v) for v in views]
    g = torch.Generator().manual_seed(5)
    for conf, pts, _ in views:
        r = torch.rand(conf.shape, generator=g).numpy()
        conf[r < 0.1] = np.nan
        conf[(r >= 0.1) & (r < 0.2)] = np.inf
        conf[(r >= 0.2) & (r < 0.25)] = -np.inf
        q = torch.rand(pts.shape, generator=g).numpy()
        pts[q < 0.03] = np.nan
        pts[(q >= 0.03) & (q < 0.06)] = np.inf
        pts[(q >= 0.06) & (q < 0.09)] = -np.inf
    M = RR.identity(2)
    cam = _cam(scene, 1)
    for thr in (1.5, float("inf")):
        want = RR.render(views, M, cam, thr)
        hit = want[2] != EMPTY
        assert hit.sum() > (200 if thr == 1.5 else 20) and np.isfinite(want[1][hit]).all()
        _equal(_render(views, None, [cam], thr)[0], want, thr)


def test_huge_coordinates_are_clipped_before_any_integer():
    """u = +-1e30, v = +-1e30 and +-2.7e41 (the largest fp32 coordinate at the near plane), beside ordinary points"""
    conf = np.full((1, 8), 2.0, dtype=np.float32)
    pts = np.array([[[0, 0, 1], [1e29, 0, 1], [-1e29, 0, 1], [0, 1e29, 1], [0, -1e29, 1], [3e38, 3e38, 0.011], [0.05, 0.05, 0.5], [-3e38, 0, 0.011]]],
                   dtype=np.float32)
    rgb = np.linspace(0, 1, 24, dtype=np.float32).reshape(1, 8, 3)
    cam = RR.Camera(np.eye(4)[:3], 10.0, 10.0, 4.0, 4.0, 8, 8, 0.01, 100.0)
    Z, u, v = RR.project(RR.compose(cam.w2c, np.eye(4)[:3]), cam, pts.reshape(-1, 3))
    assert abs(u[1] / 1e30 - 1) < 1e-6 and abs(u[2] / -1e30 - 1) < 1e-6 and abs(v[3] / 1e30 - 1) < 1e-6 and abs(v[4] / -1e30 - 1) < 1e-6
    assert u[5] > 1e41 and v[5] > 1e41 and u[7] < -1e41 and np.isfinite(u).all()
    for ps in (1, 8):
        want = RR.render([(conf, pts, rgb)], RR.identity(1), cam, 1.5, ps)
        assert set(np.unique(want[2])) == ({0, 6, EMPTY} if ps == 1 else {0, 6})
        _equal(_render([(conf, pts, rgb)], None, [cam], 1.5, ps)[0], want, ps)


def test_depth_range_ends_are_kept():
    zn, zf = np.float32(0.01), np.float32(100.0)
    z = [zn, np.nextafter(zn, np.float32(0)), zf, np.nextafter(zf, np.float32(200)), np.float32(1.0)]
    # one pixel each: u = 10 x / z + 4 with x = (k - 3.5) z / 10 up to rounding: the columns are asserted below
    pts = np.array([[[(k - 3.4) * float(zk) / 10, 0, zk] for k, zk in enumerate(z)]], dtype=np.float32)
    conf = np.full((1, 5), 2.0, dtype=np.float32)
    rgb = np.linspace(0, 1, 15, dtype=np.float32).reshape(1, 5, 3)
    cam = RR.Camera(np.eye(4)[:3], 10.0, 10.0, 4.0, 0.5, 8, 1, float(zn), float(zf))
    want = RR.render([(conf, pts, rgb)], RR.identity(1), cam, 1.5)
    assert want[2][0].tolist() == [0, EMPTY, 2, EMPTY, 4, EMPTY, EMPTY, EMPTY]
    assert want[1][0, 0] == zn and want[1][0, 2] == zf
    _equal(_render([(conf, pts, rgb)], None, [cam], 1.5)[0], want)


def test_threshold_above_every_confidence_gives_the_background():
    scene, views, _ = _scene()
    hi = max(float(c.max()) for c, _, _ in views) + 1.0
    got = _render(views, None, [_cam(scene, 0)], hi, 3, (1, 2, 3))[0]
    assert (got["index"] == EMPTY).all() and np.isposinf(got["depth"]).all() and (got["rgb"] == [1, 2, 3]).all()


def test_outputs_one_at_a_time_batches_chunks_and_repeats():
    scene, views, _ = _scene()
    M = RR.identity(len(views))
    cams = [_cam(scene, 0), _cam(scene, 1), _cam(scene, 4)]
    renderer = Rn.SceneRenderer(views, None, device=DEV)
    full = _np(renderer.render(cams, 1.5, 2))
    for i, cam in enumerate(cams[:2]):
        _equal(full[i], _want(f"batch{i}", views, M, cam, 1.5, 2), i)
    # each output alone (the others NULL)
    for k in ("rgb", "depth", "index"):
        one = _np(renderer.render(cams, 1.5, 2, want=(k,)))
        assert all(set(im) == {k} and np.array_equal(im[k].view(np.uint8), f[k].view(np.uint8)) for im, f in zip(one, full)), k
    # a camera alone, first in a batch of three and last in it
    alone = _np(renderer.render([cams[1]], 1.5, 2))[0]
    first = _np(renderer.render([cams[1], cams[0], cams[2]], 1.5, 2))[0]
    last = _np(renderer.render([cams[0], cams[2], cams[1]], 1.5, 2))[2]
    for other in (alone, first, last):
        assert all(np.array_equal(other[k].view(np.uint8), full[1][k].view(np.uint8)) for k in full[1])
    # a scratch budget of one z-buffer: three native calls
    small = Rn.SceneRenderer(views, None, device=DEV, scratch_budget=8 * 64 * 48)
    chunked = _np(small.render(cams, 1.5, 2))
    assert small.scratch.numel() < renderer.scratch.numel()
    # two runs
    again = _np(renderer.render(cams, 1.5, 2))
    for other in (chunked, again):
        assert all(np.array_equal(a[k].view(np.uint8), f[k].view(np.uint8)) for a, f in zip(other, full) for k in f)


# ---------------------------------------------------------------------------------------------------------------------------------
# stream and synchronisation (the pattern of tests/stream_forms.py: two valid input sets, the decoy in place while the call is queued)
# ---------------------------------------------------------------------------------------------------------------------------------
def _device_views(views):
    return [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in v) for v in views]


def test_render_does_not_synchronise_and_runs_on_the_callers_stream():
    from test_stream_order_gpu import Delay
    scene, views_a, _ = _scene()
    _, views_b, _ = _scene(MIXED, 9)
    cams = [_cam(scene, 0), _cam(scene, 1)]
    src = {"A": _device_views(views_a), "B": _device_views(views_b)}
    live = [tuple(torch.empty_like(t) for t in v) for v in src["A"]]
    renderer = Rn.SceneRenderer(live, None, device=DEV)
    assert all(a.data_ptr() == b.data_ptr() for va, vb in zip(renderer.tensors, live) for a, b in zip(va, vb))      # used in place

    def load(which):
        for v, s in zip(live, src[which]):
            for t, x in zip(v, s):
                t.copy_(x)

    def call():
        return [{k: v.clone() for k, v in im.items()} for im in renderer.render(cams, 1.5, 2)]

    ref = {}
    for which in ("A", "B"):
        load(which)
        ref[which] = _np(call())
    assert float((ref["A"][0]["index"] != ref["B"][0]["index"]).mean()) > 0.3
    delay = Delay()
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(40.0)
        done.record()
        load("A")
        torch.cuda.set_sync_debug_mode("error")
        try:
            t0 = time.perf_counter()
            images = renderer.render(cams, 1.5, 2)
            host_ms = (time.perf_counter() - t0) * 1e3
        finally:
            torch.cuda.set_sync_debug_mode("default")
        premise = not done.query()
        got = [{k: v.clone() for k, v in im.items()} for im in images]        # consumed on that stream
        load("B")
    s.synchronize()
    print(f"render of 2 cameras: {host_ms:.3f} ms on the host behind a 40 ms delay, premise {premise}")
    assert premise, f"the call took {host_ms:.3f} ms on the host behind a 40 ms delay: it waited for the stream"
    got = _np(got)
    for g, a in zip(got, ref["A"]):
        assert all(np.array_equal(g[k].view(np.uint8), a[k].view(np.uint8)) for k in a)


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _png(path):
    import PIL.Image
    with PIL.Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def test_render_scene_writes_the_device_pixels(tmp_path):
    scene, views, _ = _scene()
    cams = [Rn.view_camera(scene, i) for i in range(len(MIXED))] + [Rn.follow_camera(scene.cams2world[0], 40, 30)]
    paths = Rn.render_scene(str(tmp_path), scene, cams, thr=1.5, point_size=2, depth=True)
    assert [os.path.basename(p) for p in paths] == ["frame_%05d.png" % i for i in range(6)]
    assert sorted(os.listdir(tmp_path)) == sorted(["frame_%05d.png" % i for i in range(6)] + ["depth_%05d.png" % i for i in range(6)])
    images = Rn.SceneRenderer(views, None, device=DEV).render(cams, 1.5, 2)
    for i, (p, im) in enumerate(zip(paths, images)):
        assert np.array_equal(_png(p), im["rgb"].cpu().numpy()), i
        assert _png(p).shape == (cams[i].H, cams[i].W, 3)
        panel = _png(os.path.join(str(tmp_path), "depth_%05d.png" % i))
        d = im["depth"].cpu().numpy()
        hit = np.isfinite(d)
        assert np.array_equal(panel, Rn.depth_panel(im["depth"]).cpu().numpy()) and (panel[~hit] == 0).all()
        if hit.sum() > 1:
            assert panel[hit].max() == 255 and (panel[..., 0] == panel[..., 1]).all() and (panel[..., 1] == panel[..., 2]).all()
    # a view seen from its own camera (focal 10, its own size): equal to the restatement, and not empty
    want = RR.render(views, RR.identity(len(views)), RR.view_camera(scene, 0), 1.5, 2)
    assert (want[2] != EMPTY).mean() > 0.2 and np.array_equal(_png(paths[0]), want[0])


def test_orbit_cameras_enclose_the_kept_points():
    scene, views, _ = _scene()
    pos = np.concatenate([pts[R.select(conf, 1.5)] for conf, pts, _ in views])
    cams = Rn.orbit_cameras(scene, 5, 1.5, 64, 48)
    assert len(cams) == 5
    renderer = Rn.SceneRenderer(views, None, device=DEV)
    images = _np(renderer.render(cams, 1.5, 1, want=("index",)))
    for cam, im in zip(cams, images):
        X = pos.astype(np.float64) @ np.asarray(cam.w2c)[:, :3].T + np.asarray(cam.w2c)[:, 3]
        u, v = cam.fx * X[:, 0] / X[:, 2] + cam.cx, cam.fy * X[:, 1] / X[:, 2] + cam.cy
        assert (X[:, 2] > cam.z_near).all() and (X[:, 2] < cam.z_far).all() and (u >= 0).all() and (u < 64).all() and (v >= 0).all() and (v < 48).all()
        assert (im["index"] != EMPTY).sum() > 20
    with pytest.raises(ValueError):
        Rn.orbit_cameras(scene, 5, 1e9, 64, 48)


def test_colorize_grayscale():
    g = torch.Generator().manual_seed(3)
    x = torch.rand((48, 64), generator=g) * 7 + 0.5
    got = Rn.colorize_grayscale(x.to(DEV))
    xn = x.numpy()
    want = (xn - xn.min()) / (xn.max() - xn.min() + 1e-9)
    assert got.shape == (48, 64, 3) and got.dtype == torch.float32 and got.is_cuda
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - np.stack([want] * 3, -1).astype(np.float64)).max())
    print(f"colorize_grayscale: max abs difference from the numpy formula {err:.3e} (bound 4.8e-7)")
    assert err <= 4.8e-7 and float(got.min()) == 0.0


def test_get_reconstructed_scene_render_dir(tmp_path):
    import PIL.Image
    from test_asmk_gpu import _models, _pngs
    _, enc, dec = _models()
    (tmp_path / "in").mkdir()
    files = _pngs(tmp_path / "in", 5)
    args = (None, False, (enc, dec), None, DEV, False, 224, False, files, 0, 0, "linseq", 3, False, 3, 2, 3, 2, 1.5, 0.05, 70, 1.05, True, False, False, 0.05)
    out = tmp_path / "out"
    out.mkdir()
    scene, _ = Dm.get_reconstructed_scene(str(out), *args)
    assert os.listdir(out) == []                       # default: nothing new is written
    frames = tmp_path / "frames"
    scene, _ = Dm.get_reconstructed_scene(str(out), *args, render_dir=str(frames), render_views=3)
    n = len(files)
    assert n == 5 and os.listdir(out) == [] and sorted(os.listdir(frames)) == ["frame_%05d.png" % i for i in range(n + 3)]
    for i in range(n + 3):
        H, W = scene.imgs[i if i < n else 0].shape[:2]       # a view's frame has its image's size, an orbit frame image 0's
        with PIL.Image.open(frames / ("frame_%05d.png" % i)) as im:
            assert im.size == (W, H) and im.mode == "RGB"
