"""GPU (-m gpu): the scene export (must3r_amd.export / demo.get_3D_model_from_scene / demo.export_scene_thresholds) against the numpy
restatement tests/export_ref.py, bit for bit: positions, colours, order, min / max, faces, for point clouds and meshes, GLB and PLY.
Nothing here reads the reference checkout."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import export_ref as R
from must3r_amd import _lib, demo as Dm, export as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = list(R.THRESHOLDS)
MIXED = [(48, 64), (48, 64), (32, 64), (32, 64), (48, 64)]   # the tiny_mixed_ar shapes


def _counts(scene, thr):
    return sum(int(R.select(x["conf"], thr).sum()) for x in scene.x_out)


def _check_pointcloud_files(scene, paths, thresholds, file_type, local=False, cameras=None):
    views = R.scene_views(scene, local)
    M = R.view_matrices(scene.cams2world, local)
    assert len(paths) == len(thresholds)
    for path, thr in zip(paths, thresholds):
        assert os.path.basename(path) == f"scene_{thr}.{file_type}"
        pos, col = R.pointcloud(views, M, thr)
        if file_type == "ply":
            got = R.read_ply(path)
            assert got.dtype.names == ("x", "y", "z", "red", "green", "blue", "alpha")
            assert np.array_equal(got.tobytes(), R.ply_records(pos, col).tobytes())
            continue
        glb = R.read_glb(path)
        p = glb["primitives"][0]
        assert p["mode"] == 0 and p["indices"] is None
        assert np.array_equal(p["POSITION"].view(np.uint32), pos.view(np.uint32)), thr
        assert np.array_equal(p["COLOR_0"], col), thr
        acc = p["accessors"]["POSITION"]
        assert acc["min"] == [float(v) for v in pos.min(0)] and acc["max"] == [float(v) for v in pos.max(0)]
        assert p["accessors"]["COLOR_0"]["normalized"] is True and p["accessors"]["COLOR_0"]["componentType"] == 5121
        if cameras is not None:
            assert len(glb["primitives"]) == 2 and glb["primitives"][1]["mode"] == 1
            assert len(glb["primitives"][1]["POSITION"]) == 5 * cameras


@pytest.mark.parametrize("file_type", ["glb", "ply"])
@pytest.mark.parametrize("name,shapes", [("one", [(48, 64)]), ("mixed", MIXED), ("ragged", [(7, 13), (33, 37), (1, 5), (40, 64)])])
def test_pointcloud_thresholds_equal_restatement(tmp_path, name, shapes, file_type):
    scene = R.make_scene(shapes, seed=0)
    n = sum(h * w for h, w in shapes)
    if name == "mixed":
        for thr in THR:
            assert 0 < _counts(scene, thr) < n, thr      # every reference threshold selects a non-empty, non-full subset
    thresholds = [t for t in THR if _counts(scene, t) > 0]
    assert len(thresholds) >= 6
    paths = Dm.export_scene_thresholds(str(tmp_path), scene, THR, file_type=file_type)
    _check_pointcloud_files(scene, paths, thresholds, file_type, cameras=len(shapes))


def test_thresholds_above_and_below_every_confidence(tmp_path):
    scene = R.make_scene(MIXED, seed=1)
    hi = max(float(x["conf"].max()) for x in scene.x_out) + 1.0
    with pytest.raises(ValueError):
        Dm.get_3D_model_from_scene(str(tmp_path), False, scene, min_conf_thr=hi, as_pointcloud=True, filename="none.glb")
    assert os.listdir(tmp_path) == []
    paths = Dm.export_scene_thresholds(str(tmp_path), scene, [hi, 0.5, hi + 1], file_type="glb")
    assert [os.path.basename(p) for p in paths] == ["scene_0.5.glb"] and sorted(os.listdir(tmp_path)) == ["scene_0.5.glb"]
    p = R.read_glb(paths[0])["primitives"][0]
    pos, col = R.pointcloud(R.scene_views(scene), R.view_matrices(scene.cams2world, False), 0.5)
    assert len(pos) == sum(h * w for h, w in MIXED)
    assert np.array_equal(p["POSITION"].view(np.uint32), pos.view(np.uint32)) and np.array_equal(p["COLOR_0"], col)


def test_nan_and_inf_confidences(tmp_path):
    scene = R.make_scene([(33, 37), (48, 64)], seed=2)
    g = torch.Generator().manual_seed(5)
    for x in scene.x_out:
        r = torch.rand(x["conf"].shape, generator=g)
        x["conf"][r < 0.1] = float("nan")
        x["conf"][(r >= 0.1) & (r < 0.2)] = float("inf")
        x["conf"][(r >= 0.2) & (r < 0.25)] = float("-inf")
    thresholds = [3.0, 1.05, float("inf")]
    n_inf = sum(int(torch.isposinf(x["conf"]).sum()) for x in scene.x_out)
    assert n_inf > 0 and _counts(scene, float("inf")) == n_inf
    paths = Dm.export_scene_thresholds(str(tmp_path), scene, thresholds, file_type="ply")
    _check_pointcloud_files(scene, paths, thresholds, "ply")
    assert len(R.read_ply(paths[2])) == n_inf


@pytest.mark.parametrize("file_type", ["glb", "ply"])
def test_host_and_device_resident_scenes_give_identical_bytes(tmp_path, file_type):
    host, dev = R.make_scene(MIXED, seed=3), R.make_scene(MIXED, seed=3, device=DEV)
    assert dev.x_out[0]["conf"].is_cuda and dev.imgs[0].is_cuda
    a = Dm.export_scene_thresholds(str(tmp_path / "host"), host, THR, file_type=file_type, local_pointmaps=True)
    b = Dm.export_scene_thresholds(str(tmp_path / "dev"), dev, THR, file_type=file_type, local_pointmaps=True)
    assert len(a) == len(b) == 8
    for pa, pb in zip(a, b):
        assert open(pa, "rb").read() == open(pb, "rb").read()


@pytest.mark.parametrize("local", [False, True])
def test_local_pointmaps_equal_restatement(tmp_path, local):
    scene = R.make_scene(MIXED, seed=4)
    paths = Dm.export_scene_thresholds(str(tmp_path), scene, THR, file_type="glb", local_pointmaps=local, camera_conf_thr=2.015)
    kept = sum(bool(x["conf"].median() >= 2.015) for x in scene.x_out)
    assert 0 < kept < len(MIXED)
    _check_pointcloud_files(scene, paths, THR, "glb", local=local, cameras=kept)


def _mask_scene(kind, shapes, seed):
    scene = R.make_scene(shapes, seed=seed)
    for x in scene.x_out:
        H, W = x["conf"].shape
        if kind == "checkerboard":
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            x["conf"] = torch.where((yy + xx) % 2 == 0, torch.tensor(5.0), torch.tensor(1.0))
        elif kind == "all":
            x["conf"] = torch.full((H, W), 5.0)
    return scene


@pytest.mark.parametrize("kind", ["checkerboard", "all", "random"])
def test_mesh_equals_restatement(tmp_path, kind):
    shapes = [(48, 64), (33, 37), (7, 13)]
    scene = _mask_scene(kind, shapes, seed=6)
    thresholds = [3.0] if kind != "random" else THR
    views, M = R.scene_views(scene), R.view_matrices(scene.cams2world, False)
    if kind == "checkerboard":
        assert len(R.mesh(views, M, 3.0)[2]) == 0
        with pytest.raises(ValueError):
            Dm.get_3D_model_from_scene(str(tmp_path), False, scene, min_conf_thr=3.0, as_pointcloud=False)
        assert os.listdir(tmp_path) == []
        return
    paths = Dm.export_scene_thresholds(str(tmp_path), scene, thresholds, file_type="glb", as_pointcloud=False)
    assert len(paths) == len(thresholds)
    for path, thr in zip(paths, thresholds):
        pos, col, faces = R.mesh(views, M, thr)
        if kind == "all":
            assert len(faces) == sum(4 * (h - 1) * (w - 1) for h, w in shapes)
        else:
            assert 0 < len(faces) < sum(4 * (h - 1) * (w - 1) for h, w in shapes)
        p = R.read_glb(path)["primitives"][0]
        assert p["mode"] == 4 and p["material"]["doubleSided"] is True
        assert p["indices"].dtype == np.uint32 and np.array_equal(p["indices"].reshape(-1, 3), faces), thr
        assert np.array_equal(p["POSITION"].view(np.uint32), pos.view(np.uint32)) and np.array_equal(p["COLOR_0"], col)
        acc = p["accessors"]["POSITION"]
        assert acc["min"] == [float(v) for v in pos.min(0)] and acc["max"] == [float(v) for v in pos.max(0)]


@pytest.mark.parametrize("as_pointcloud,file_type", [(True, "glb"), (True, "ply"), (False, "glb")])
def test_single_threshold_call_writes_the_same_bytes(tmp_path, as_pointcloud, file_type):
    scene = R.make_scene(MIXED, seed=7)
    multi = Dm.export_scene_thresholds(str(tmp_path / "multi"), scene, THR, file_type=file_type, as_pointcloud=as_pointcloud)
    assert len(multi) == 8
    for thr, pm in zip(THR, multi):
        one = Dm.get_3D_model_from_scene(str(tmp_path / "one"), False, scene, min_conf_thr=thr, as_pointcloud=as_pointcloud,
                                         filename=f"s_{thr}.{file_type}")
        assert one == str(tmp_path / "one" / f"s_{thr}.{file_type}")
        assert open(one, "rb").read() == open(pm, "rb").read(), thr


def test_more_than_eight_thresholds_are_chunked(tmp_path):
    scene = R.make_scene(MIXED, seed=8)
    thresholds = [1.0 + 0.25 * i for i in range(11)]
    paths = Dm.export_scene_thresholds(str(tmp_path), scene, thresholds, file_type="ply")
    _check_pointcloud_files(scene, paths, thresholds, "ply")


def test_ply_refuses_mesh_and_none_scene(tmp_path):
    scene = R.make_scene([(8, 8)], seed=9)
    with pytest.raises(ValueError):
        Dm.get_3D_model_from_scene(str(tmp_path), False, scene, as_pointcloud=False, filename="scene.ply")
    assert Dm.get_3D_model_from_scene(str(tmp_path), False, None) is None


def test_scale_200_views_on_device():
    """200 views of 384 x 512 (39.3 M points), eight thresholds from one count: every packed buffer and min / max equal a torch
    restatement computed on the device (fp64 ops one by one, torch does not fuse them in eager mode)."""
    V, H, W = 200, 384, 512
    g = torch.Generator(device=DEV).manual_seed(0)
    conf = 1.0 + torch.exp(torch.randn((V, H, W), generator=g, device=DEV))
    pts = torch.randn((V, H, W, 3), generator=g, device=DEV)
    rgb = torch.rand((V, H, W, 3), generator=g, device=DEV) * 1.2 - 0.1
    gm = torch.Generator().manual_seed(1)
    M = torch.randn((V, 3, 4), generator=gm, dtype=torch.float64)
    ex = E.SceneExporter([(conf[i], pts[i], rgb[i]) for i in range(V)], M.numpy())
    totals = ex.count(THR)
    Md = M.to(DEV)
    pos_all = torch.empty((V, H, W, 3), dtype=torch.float32, device=DEV)
    for i in range(V):
        p = pts[i].double()
        for a in range(3):
            m = Md[i, a]
            pos_all[i, ..., a] = (((m[0] * p[..., 0] + m[1] * p[..., 1]) + m[2] * p[..., 2]) + m[3]).float()
    col_all = torch.round(rgb.clamp(0, 1) * 255).to(torch.uint8)
    col_all = torch.cat([col_all, torch.full((V, H, W, 1), 255, dtype=torch.uint8, device=DEV)], dim=-1)
    for k, thr in enumerate(THR):
        mask = conf >= thr
        n = int(mask.sum())
        assert totals[k] == n and 0 < n < V * H * W
        want_pos, want_col = pos_all[mask], col_all[mask]
        buf, got_n, mm = ex.points_device(k, _lib.EXPORT_GLB)
        assert got_n == n
        assert torch.equal(buf[:12 * n].view(torch.float32).view(n, 3), want_pos), thr
        assert torch.equal(buf[12 * n:16 * n].view(n, 4), want_col), thr
        assert torch.equal(mm[:3], want_pos.amin(0)) and torch.equal(mm[3:], want_pos.amax(0))
        buf, _, _ = ex.points_device(k, _lib.EXPORT_PLY)
        rec = buf.view(n, 16)
        assert torch.equal(rec[:, :12].contiguous().view(torch.float32).view(n, 3), want_pos), thr
        assert torch.equal(rec[:, 12:], want_col), thr
        del want_pos, want_col, mask


def test_end_to_end_from_images(tmp_path):
    from test_asmk_gpu import _models, _pngs
    _, enc, dec = _models()
    files = _pngs(tmp_path, 5)
    scene, _ = Dm.get_reconstructed_scene(
        str(tmp_path), None, False, (enc, dec), None, DEV, False, 224, False, files, 0, 0, "linseq", 3, False, 3, 2, 3, 2, 1.5, 0.05, 70,
        3.0, True, False, False, 0.05)
    lo = min(float(x["conf"].min()) for x in scene.x_out)
    hi = max(float(x["conf"].max()) for x in scene.x_out)
    thresholds = THR + [lo, 0.5 * (lo + hi)]
    for file_type in ("glb", "ply"):
        out = tmp_path / file_type
        paths = Dm.export_scene_thresholds(str(out), scene, thresholds, file_type=file_type)
        want = {f"scene_{t}.{file_type}": _counts(scene, t) for t in thresholds if _counts(scene, t) > 0}
        assert f"scene_{lo}.{file_type}" in want and sorted(os.path.basename(p) for p in paths) == sorted(want)
        for p in paths:
            n = len(R.read_ply(p)) if file_type == "ply" else len(R.read_glb(p)["primitives"][0]["POSITION"])
            assert n == want[os.path.basename(p)], p


def test_c_abi_refusals():
    lib = _lib.load()
    conf = torch.ones((4, 4), device=DEV)
    pts = torch.ones((4, 4, 3), device=DEV)
    table = (_lib.ExportView * 3)()
    for e in table:
        e.conf, e.pts, e.rgb, e.H, e.W = conf.data_ptr(), pts.data_ptr(), pts.data_ptr(), 4, 4
    thr = (C.c_float * 9)(*([1.0] * 9))
    totals = (C.c_int64 * 9)()
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    sp, stream = C.c_void_p(scratch.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(rc, word):
        assert rc != 0
        msg = lib.must3r_hip_last_error().decode()
        assert word in msg, msg

    assert lib.must3r_hip_export_scratch_bytes(table, 3, 8, 0) > 0
    assert lib.must3r_hip_export_scratch_bytes(table, 3, 9, 0) == 0
    refused(lib.must3r_hip_export_count(table, 3, thr, 9, 0, sp, scratch.numel(), totals, stream), "thresholds")
    refused(lib.must3r_hip_export_count(None, 3, thr, 8, 0, sp, scratch.numel(), totals, stream), "null view table")
    # 2^32 vertices: arithmetic on the sizes alone, nothing that large is allocated or read
    for e in table:
        e.H, e.W = 32768, 43691
    assert 3 * 32768 * 43691 >= 2 ** 32 > 2 * 32768 * 43691
    refused(lib.must3r_hip_export_count(table, 3, thr, 8, 0, sp, scratch.numel(), totals, stream), "2^32")
    assert lib.must3r_hip_export_scratch_bytes(table, 3, 8, 1) == 0
    assert lib.must3r_hip_export_scratch_bytes(table, 2, 8, 0) > 0
    table[0].H, table[0].W = 65536, 32768          # one view of 2^31 pixels: the kernels index a view's pixels in 32 bits
    refused(lib.must3r_hip_export_count(table, 1, thr, 8, 0, sp, scratch.numel(), totals, stream), "2^31")
    torch.cuda.synchronize()
