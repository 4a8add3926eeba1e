"""GPU (-m gpu): the mesh rasteriser (must3r_amd.render with ``mesh=True`` / csrc/render_mesh.hip) against the numpy restatement
tests/render_mesh_ref.py, bit for bit: colour, depth and triangle id of every target pixel, on the cases of tests/render_mesh_cases.py (that they are
not vacuous is shown on the CPU, tests/test_render_mesh_host.py).  Nothing here reads the reference checkout."""
import os
import time

import numpy as np
import pytest
import torch

import export_ref as R
import render_mesh_cases as K
import render_ref as RR
from must3r_amd import _lib, demo as Dm, render as Rn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMPTY = 0xFFFFFFFF
SIZES = lambda: K.sizes_case(_lib.RENDER_MESH_WAVE_AREA)   # noqa: E731


def _host(images):
    torch.cuda.synchronize()
    return [{k: v.cpu() for k, v in im.items()} for im in images]


def _render(views, matrices, cams, thr, mesh=True, ps=1, bg=(255, 255, 255), want=("rgb", "depth", "index"), **kw):
    M = None if matrices is None else np.stack([np.asarray(m, dtype=np.float64) for m in matrices])
    return _host(Rn.SceneRenderer(views, M, device=DEV, **kw).render(cams, thr, ps, bg, want, mesh=mesh))


def _t(x):
    """a numpy image as the int32 / uint8 tensor whose bits torch.equal compares"""
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype.itemsize == 4 else np.uint8))


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.int32 if a[k].element_size() == 4 else torch.uint8),
                                                b[k].view(torch.int32 if b[k].element_size() == 4 else torch.uint8)) for k in a)


def _equal(got, want, what=""):
    rgb, depth, index = want[:3]
    assert got["index"].dtype == torch.uint32 and got["depth"].dtype == torch.float32 and got["rgb"].dtype == torch.uint8
    assert torch.equal(got["index"].view(torch.int32), _t(index)), what
    assert torch.equal(got["depth"].view(torch.int32), _t(depth)), what
    assert torch.equal(got["rgb"], _t(rgb)), what


def _case_equals(name, builder):
    views, M, cams, thr = K.case(name, builder)
    got = _render(views, M, cams, thr)
    for ci in range(len(cams)):
        _equal(got[ci], K.want(name, builder, ci), f"{name}, camera {ci}")
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_main_case_equals_restatement():
    views, M, cams, thr = K.case("main", K.main_case)
    # on the restatement alone first: no part is vacuous
    reasons = dict.fromkeys(("conf", "nonfinite", "near", "far", "off_image", "clipped"), 0)
    for ci, cam in enumerate(cams):
        c = K.want("main", K.main_case, ci)[3]
        cnt = np.bincount(c["pix"], minlength=cam.W * cam.H)
        print(f"camera {ci}: covered {(cnt > 0).mean():.3f}, two or more contenders {(cnt >= 2).mean():.3f}, {c['stats']}")
        assert (cnt > 0).mean() >= 1 / 3 and (cnt >= 2).sum() >= 1
        for k in reasons:
            reasons[k] += c["stats"][k]
    assert all(v >= 1 for v in reasons.values()), reasons
    got = _case_equals("main", K.main_case)
    assert got[0]["rgb"].shape == (30, 40, 3) and got[0]["depth"].shape == (30, 40) and got[0]["index"].shape == (30, 40)


def test_edges_and_vertices_on_sample_points():
    got = _case_equals("lattice", K.lattice_case)[0]
    covered = torch.zeros((8, 8), dtype=torch.bool)
    covered[:7, :7] = True                    # every centre in or on the outline, vertices and diagonals included
    assert torch.equal(got["index"].view(torch.int32) != -1, covered)
    planted = K.want("lattice", K.lattice_case, 0, exclusive=True)
    assert not torch.equal(got["index"].view(torch.int32), _t(planted[2]))


def test_watertight_where_points_leave_holes():
    views, M, cams, thr = K.case("plane", K.plane_case)
    got = _case_equals("plane", K.plane_case)[0]
    inside = torch.from_numpy(K.inside_outline(K.plane_outline(views, M, cams[0]), 64, 48, 1.0))
    hit = got["index"].view(torch.int32) != -1
    assert int(inside.sum()) > 1000 and bool(hit[inside].all())
    points = _render(views, M, cams, thr, mesh=False)[0]["index"].view(torch.int32) != -1
    print(f"inside the outline: {int(inside.sum())} pixels, mesh covers {int(hit[inside].sum())}, points of size 1 cover {int(points[inside].sum())}")
    assert int(points[inside].sum()) < int(inside.sum()) // 4


def test_both_size_paths():
    wa = _lib.RENDER_MESH_WAVE_AREA
    areas = []
    for ci in range(4):
        boxes = K.want("sizes", SIZES, ci)[3]["boxes"]
        areas.append([(b[1] - b[0] + 1) * (b[3] - b[2] + 1) for b in (boxes[0], boxes[1])])
    assert areas == [[wa - 1] * 2, [wa] * 2, [wa + 1] * 2, [256] * 2]
    got = _case_equals("sizes", SIZES)
    assert bool((got[3]["index"].view(torch.int32) == 0).all())          # one triangle covers the whole target
    # and two source blocks whose waves hold many large triangles at once beside small ones
    areas = np.array([(b[1] - b[0] + 1) * (b[3] - b[2] + 1) for b in K.want("blocks", K.blocks_case, 1)[3]["boxes"].values()])
    assert (areas > wa).sum() >= 20 and (areas <= wa).sum() >= 20
    _case_equals("blocks", K.blocks_case)


def test_degenerate_triangles_draw_nothing():
    c = K.want("degenerate", K.degenerate_case, 0)[3]
    assert c["stats"]["drawn"] >= 3 and len(c["pix"]) == 0
    got = _case_equals("degenerate", K.degenerate_case)[0]
    assert bool((got["index"].view(torch.int32) == -1).all()) and bool(torch.isposinf(got["depth"]).all()) and bool((got["rgb"] == 255).all())


def test_ties_order_repeats_batches_and_chunks():
    views, M, cams, thr = K.case("twin", K.twin_case)
    got = _case_equals("twin", K.twin_case)[0]
    hit = got["index"].view(torch.int32) != -1
    n = 6 * 7
    assert float(hit.float().mean()) > 0.1 and int(got["index"].view(torch.int32)[hit].max()) < 2 * n       # the lower id wins every tie
    # the views swapped: the same ids and depths, the other view's colours
    swapped = _render(views[::-1], M, cams, thr)[0]
    assert torch.equal(swapped["index"].view(torch.int32), got["index"].view(torch.int32)) and torch.equal(swapped["depth"], got["depth"])
    assert not torch.equal(swapped["rgb"], got["rgb"])
    _equal(swapped, RR_mesh(views[::-1], M, cams[0], thr))
    # two runs, each camera alone, a scratch budget of one z-buffer
    views, M, cams, thr = K.case("main", K.main_case)
    Mx = np.stack(M)
    renderer = Rn.SceneRenderer(views, Mx, device=DEV)
    full = _host(renderer.render(cams, thr, mesh=True))
    again = _host(renderer.render(cams, thr, mesh=True))
    small = Rn.SceneRenderer(views, Mx, device=DEV, scratch_budget=8 * 40 * 30)
    chunked = _host(small.render(cams, thr, mesh=True))
    assert small.scratch.numel() < renderer.scratch.numel()
    for ci, cam in enumerate(cams):
        alone = _host(renderer.render([cam], thr, mesh=True))[0]
        last = _host(renderer.render([cams[(ci + 1) % 3], cams[(ci + 2) % 3], cam], thr, mesh=True))[2]
        assert all(_same(o, full[ci]) for o in (again[ci], chunked[ci], alone, last)), ci


def RR_mesh(views, M, cam, thr):
    import render_mesh_ref as MR
    return MR.render(views, M, cam, thr)


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
def test_want_subsets_and_point_mode_beside_it():
    views, M, cams, thr = K.case("main", K.main_case)
    renderer = Rn.SceneRenderer(views, np.stack(M), device=DEV)
    full = _host(renderer.render(cams, thr, mesh=True, background=(9, 8, 7)))
    assert bool((full[0]["rgb"][full[0]["index"].view(torch.int32) == -1] == torch.tensor([9, 8, 7], dtype=torch.uint8)).all())
    for want in (("rgb",), ("depth",), ("index",), ("rgb", "index")):
        one = _host(renderer.render(cams, thr, mesh=True, background=(9, 8, 7), want=want))
        assert all(set(im) == set(want) and _same(im, {k: f[k] for k in want}) for im, f in zip(one, full)), want
    # the same renderer in point mode between two mesh calls: the restatement of the point path, untouched
    pts = _host(renderer.render(cams[:1], thr, 2))[0]
    want = RR.render(views, M, cams[0], thr, 2)
    _equal(pts, want)
    with pytest.raises(ValueError, match="mesh=True"):
        renderer.render(cams, thr, 2, mesh=True)


def _device_views(views):
    return [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in v) for v in views]


def test_mesh_render_does_not_synchronise_and_runs_on_the_callers_stream():
    """the pattern of tests/test_render_gpu.py: two valid input sets, the decoy in place while the call is queued behind a delay on a side stream"""
    from test_stream_order_gpu import Delay
    views_a, M, cams, thr = K.case("main", K.main_case)
    views_b = [(c, (p + np.float32(0.07)).astype(np.float32), (1.0 - r).astype(np.float32)) for c, p, r in views_a]
    src = {"A": _device_views(views_a), "B": _device_views(views_b)}
    live = [tuple(torch.empty_like(t) for t in v) for v in src["A"]]
    renderer = Rn.SceneRenderer(live, np.stack(M), device=DEV)
    assert all(a.data_ptr() == b.data_ptr() for va, vb in zip(renderer.tensors, live) for a, b in zip(va, vb))      # used in place

    def load(which):
        for v, s in zip(live, src[which]):
            for t, x in zip(v, s):
                t.copy_(x)

    ref = {}
    for which in ("A", "B"):
        load(which)
        ref[which] = _host([{k: v.clone() for k, v in im.items()} for im in renderer.render(cams, thr, mesh=True)])
    _equal(ref["A"][0], K.want("main", K.main_case, 0))
    assert not torch.equal(ref["A"][0]["rgb"], ref["B"][0]["rgb"]) and not torch.equal(ref["A"][0]["depth"], ref["B"][0]["depth"])
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
            images = renderer.render(cams, thr, mesh=True)
            host_ms = (time.perf_counter() - t0) * 1e3
        finally:
            torch.cuda.set_sync_debug_mode("default")
        premise = not done.query()
        got = [{k: v.clone() for k, v in im.items()} for im in images]        # consumed on that stream
        load("B")
    s.synchronize()
    print(f"mesh render of 3 cameras: {host_ms:.3f} ms on the host behind a 40 ms delay, premise {premise}")
    assert premise, f"the call took {host_ms:.3f} ms on the host behind a 40 ms delay: it waited for the stream"
    for g, a in zip(_host(got), ref["A"]):
        assert _same(g, a)


def _png(path):
    import PIL.Image
    with PIL.Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def test_render_scene_mesh_writes_the_device_pixels(tmp_path):
    scene = R.make_scene([(12, 16), (9, 16)], seed=3)
    views = R.scene_views(scene, False)
    cams = [Rn.view_camera(scene, i) for i in range(2)] + [Rn.follow_camera(scene.cams2world[0], 40, 30)]
    paths = Rn.render_scene(str(tmp_path), scene, cams, thr=1.5, depth=True, mesh=True)
    assert [os.path.basename(p) for p in paths] == ["frame_%05d.png" % i for i in range(3)]
    assert sorted(os.listdir(tmp_path)) == sorted(["frame_%05d.png" % i for i in range(3)] + ["depth_%05d.png" % i for i in range(3)])
    images = _host(Rn.SceneRenderer(views, None, device=DEV).render(cams, 1.5, mesh=True))
    drawn = 0
    for i, (p, im) in enumerate(zip(paths, images)):
        assert np.array_equal(_png(p), im["rgb"].numpy()) and _png(p).shape == (cams[i].H, cams[i].W, 3), i
        assert np.array_equal(_png(os.path.join(str(tmp_path), "depth_%05d.png" % i)), Rn.depth_panel(im["depth"].to(DEV)).cpu().numpy())
        drawn += int((im["index"].view(torch.int32) != -1).sum())
    assert drawn > 20
    _equal(images[0], RR_mesh(views, RR.identity(2), RR.view_camera(scene, 0), 1.5))


def test_get_reconstructed_scene_render_mesh(tmp_path):
    import PIL.Image
    from test_asmk_gpu import _models, _pngs
    _, enc, dec = _models()
    (tmp_path / "in").mkdir()
    files = _pngs(tmp_path / "in", 5)
    args = (None, False, (enc, dec), None, DEV, False, 224, False, files, 0, 0, "linseq", 3, False, 3, 2, 3, 2, 1.5, 0.05, 70, 1.05, True, False, False, 0.05)
    out = tmp_path / "out"
    out.mkdir()
    frames, frames_pts = tmp_path / "mesh", tmp_path / "points"
    scene, _ = Dm.get_reconstructed_scene(str(out), *args, render_dir=str(frames), render_views=2, render_mesh=True)
    n = len(files)
    assert os.listdir(out) == [] and sorted(os.listdir(frames)) == ["frame_%05d.png" % i for i in range(n + 2)]
    Dm.render_previews(str(frames_pts), scene, 1.05, 2)
    differ = 0
    for i in range(n + 2):
        H, W = scene.imgs[i if i < n else 0].shape[:2]
        with PIL.Image.open(frames / ("frame_%05d.png" % i)) as im:
            assert im.size == (W, H) and im.mode == "RGB"
        differ += int(not np.array_equal(_png(frames / ("frame_%05d.png" % i)), _png(frames_pts / ("frame_%05d.png" % i))))
    assert differ > 0                         # the switch reached the renderer: the mesh frames are not the point frames
    # a view's mesh frame is the renderer's own
    views = Rn.scene_views(scene, False)
    im = Rn.SceneRenderer(views, None, device=DEV).render([Rn.view_camera(scene, 0)], 1.05, mesh=True)[0]
    assert np.array_equal(_png(frames / "frame_00000.png"), im["rgb"].cpu().numpy())
