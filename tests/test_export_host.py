"""Host side of the scene export (must3r_amd.export, demo.get_3D_model_from_scene, get_reconstruction's parser), no GPU needed:
the containers read back by the independent reader of tests/export_ref.py, the scene transform against numpy and a hand-made pose, and
the reference's own get_3D_model_from_scene / _convert_scene_output_to_glb (compiled alone out of demo/gradio.py, with a recording
stand-in for trimesh) as the oracle for what is selected, in which order, which cameras are kept and which matrix is applied."""
import argparse
import ast
import os

import numpy as np
import pytest
import torch

import export_ref as R
from must3r_amd import demo as Dm, export as E
from must3r_amd import get_reconstruction as G

from oracle.ref_shims import REFERENCE_ROOT

REF_GRADIO = os.path.join(REFERENCE_ROOT, "must3r", "demo", "gradio.py")
REF_CLI = os.path.join(REFERENCE_ROOT, "get_reconstruction.py")
needs_reference = pytest.mark.skipif(not os.path.exists(REF_GRADIO), reason="the reference checkout is not present")
SHAPES = [(12, 16), (9, 16), (12, 16), (7, 5)]


# ---------------------------------------------------------------------------------------------------------------------------------
# containers
# ---------------------------------------------------------------------------------------------------------------------------------
def _arrays(thr=2.0, local=False):
    scene = R.make_scene(SHAPES, seed=11)
    views, M = R.scene_views(scene, local), R.view_matrices(scene.cams2world, local)
    return scene, views, M


def _container_rules(path, glb):
    assert glb["length"] == os.path.getsize(path)
    assert all(n % 4 == 0 for _, n in glb["chunks"])
    assert all(v["byteOffset"] % 4 == 0 for v in glb["json"]["bufferViews"])


@pytest.mark.parametrize("n_points", [1, 2, 3, 257])     # colour plane lengths 4 n, position planes 12 n: JSON padding varies with n
def test_glb_pointcloud_roundtrip(tmp_path, n_points):
    _, views, M = _arrays()
    pos, col = R.pointcloud(views, M, 1.5)
    pos, col = pos[:n_points], col[:n_points]
    path = E.write_glb(str(tmp_path / "p.glb"), pos, col, pos.min(0), pos.max(0))
    glb = R.read_glb(path)
    _container_rules(path, glb)
    assert len(glb["primitives"]) == 1
    p = glb["primitives"][0]
    assert p["mode"] == 0 and p["indices"] is None and p["material"] is None
    assert np.array_equal(p["POSITION"].view(np.uint32), pos.view(np.uint32)) and np.array_equal(p["COLOR_0"], col)
    acc = p["accessors"]
    assert acc["POSITION"]["componentType"] == 5126 and acc["POSITION"]["type"] == "VEC3"
    assert acc["POSITION"]["min"] == [float(v) for v in pos.min(0)] and acc["POSITION"]["max"] == [float(v) for v in pos.max(0)]
    assert acc["COLOR_0"] == dict(bufferView=1, componentType=5121, count=n_points, type="VEC4", normalized=True)
    assert not os.path.exists(path + ".part")


def test_glb_mesh_with_cameras_roundtrip(tmp_path):
    scene, views, M = _arrays()
    pos, col, faces = R.mesh(views, M, 2.0)
    assert len(faces) > 0
    S = E.scene_transform(scene.cams2world[0])
    cams = E.camera_frustums(scene, S, 0.05, [True, False, True, True])
    path = E.write_glb(str(tmp_path / "m.glb"), pos, col, pos.min(0), pos.max(0), faces=faces, cameras=cams)
    glb = R.read_glb(path)
    _container_rules(path, glb)
    m, c = glb["primitives"]
    assert m["mode"] == 4 and m["material"]["doubleSided"] is True
    assert m["indices"].dtype == np.uint32 and np.array_equal(m["indices"].reshape(-1, 3), faces)
    assert np.array_equal(m["POSITION"].view(np.uint32), pos.view(np.uint32)) and np.array_equal(m["COLOR_0"], col)
    assert c["mode"] == 1 and len(c["POSITION"]) == 15 and len(c["indices"]) == 48 and int(c["indices"].max()) == 14
    assert np.array_equal(c["COLOR_0"][::5, :3], np.array([E.CAM_COLORS[0], E.CAM_COLORS[2], E.CAM_COLORS[3]], dtype=np.uint8))
    assert c["accessors"]["POSITION"]["min"] == [float(v) for v in c["POSITION"].min(0)]


def test_ply_roundtrip(tmp_path):
    _, views, M = _arrays()
    pos, col = R.pointcloud(views, M, 1.5)
    rec = R.ply_records(pos, col)
    assert rec.dtype.itemsize == 16 and rec.dtype == E.PLY_DTYPE
    path = E.write_ply(str(tmp_path / "p.ply"), rec)
    got = R.read_ply(path)
    assert got.dtype.names == ("x", "y", "z", "red", "green", "blue", "alpha") and len(got) == len(pos)
    assert np.array_equal(np.stack([got["x"], got["y"], got["z"]], 1).view(np.uint32), pos.view(np.uint32))
    assert np.array_equal(np.stack([got["red"], got["green"], got["blue"], got["alpha"]], 1), col)
    raw = open(path, "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\n") and raw.endswith(rec.tobytes())


# ---------------------------------------------------------------------------------------------------------------------------------
# scene transform
# ---------------------------------------------------------------------------------------------------------------------------------
def test_scene_transform_against_numpy():
    scene = R.make_scene(SHAPES, seed=12)
    c0 = scene.cams2world[0].double().numpy()
    rot = np.diag([-1.0, 1.0, -1.0, 1.0])
    want = np.linalg.inv(c0 @ np.diag([1.0, -1.0, -1.0, 1.0]) @ rot)
    S = E.scene_transform(scene.cams2world[0])
    assert S.dtype == np.float64 and np.allclose(S, want, rtol=0, atol=1e-14)
    assert np.array_equal(S, R.scene_transform(scene.cams2world[0]))
    S2, M = E.view_matrices(scene.cams2world, local_pointmaps=False)
    assert np.array_equal(S2, S) and M.shape == (4, 3, 4) and all(np.array_equal(m, S[:3]) for m in M)
    _, Ml = E.view_matrices(scene.cams2world, local_pointmaps=True)
    for m, c in zip(Ml, scene.cams2world):
        assert np.array_equal(m, (S @ c.double().numpy())[:3])
    assert all(np.array_equal(a, b) for a, b in zip(Ml, R.view_matrices(scene.cams2world, True)))


def test_scene_transform_signs_by_hand():
    """camera 0 at the identity: S = inv(diag(1,-1,-1,1) @ rot_y(180)) = inv(diag(-1,-1,1,1)), so (x, y, z) lands at (-x, -y, z);
    a camera translated by t first has t removed: with c2w_0 = [I | (1, 2, 3)] the point (x, y, z) lands at (-(x-1), -(y-2), z-3).
    (scipy's 180 degree rotation carries sin(pi) = 1.2e-16 off the diagonal; the points avoid exact cancellation to 0, where that term
    would be all that is left, and everywhere else it vanishes in the rounding to fp32.)"""
    assert np.array_equal(E.OPENGL, np.diag([1.0, -1.0, -1.0, 1.0]))
    S = E.scene_transform(torch.eye(4))
    assert np.allclose(S, np.diag([-1.0, -1.0, 1.0, 1.0]), rtol=0, atol=2e-16)
    p = np.array([[0.5, -2.0, 3.0], [1.0, 2.0, 4.0]], dtype=np.float32)
    assert np.array_equal(R.transform(S[:3], p), np.array([[-0.5, 2.0, 3.0], [-1.0, -2.0, 4.0]], dtype=np.float32))
    c = torch.eye(4)
    c[:3, 3] = torch.tensor([1.0, 2.0, 3.0])
    p2 = np.array([[3.0, 5.0, 7.0], [-2.0, 0.5, 10.0]], dtype=np.float32)
    assert np.array_equal(R.transform(E.scene_transform(c)[:3], p2), np.array([[-2.0, -3.0, 4.0], [3.0, 1.5, 7.0]], dtype=np.float32))


def test_camera_mask_and_frustum():
    scene = R.make_scene(SHAPES, seed=13)
    med = [float(x["conf"].median()) for x in scene.x_out]
    thr = sorted(med)[2]
    assert E.camera_mask(scene.x_out, thr) == [m >= thr for m in med] and sum(E.camera_mask(scene.x_out, thr)) == 2
    v, c, idx = E.camera_frustums(scene, np.eye(4), 0.1, [False, True, False, False])
    H, W = SHAPES[1]
    c2w, f = scene.cams2world[1].double().numpy(), scene.focals[1]
    assert np.array_equal(v[0], c2w[:3, 3].astype(np.float32))            # apex = the camera centre
    corner = c2w @ np.array([0.5 * W / f * 0.1, 0.5 * H / f * 0.1, 0.1, 1.0])
    assert np.allclose(v[3], corner[:3], rtol=1e-6, atol=1e-7)
    assert idx.tolist() == [0, 1, 0, 2, 0, 3, 0, 4, 1, 2, 2, 3, 3, 4, 4, 1] and (c[:, :3] == E.CAM_COLORS[1]).all() and (c[:, 3] == 255).all()
    assert E.camera_frustums(scene, np.eye(4), 0.1, [False] * 4) is None
    assert len(E.CAM_COLORS) == 11


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's get_3D_model_from_scene / _convert_scene_output_to_glb, compiled alone (their module needs gradio, trimesh, viser)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Trimesh:
    """records what the reference hands to trimesh"""

    def __init__(self):
        self.log = []
        outer = self

        class Geometry:
            def __init__(self, kind, **kw):
                self.kind, self.kw = kind, kw

            def export(self, file_obj=None, file_type=None):
                outer.log.append(("export_geometry", self.kind, file_obj, file_type))

        class Scene:
            def __init__(self):
                self.geometry = []

            def add_geometry(self, g):
                self.geometry.append(g)
                outer.log.append(("add_geometry", g.kind, g.kw))

            def apply_transform(self, T):
                outer.log.append(("apply_transform", np.array(T)))

            def export(self, file_obj=None):
                outer.log.append(("export_scene", file_obj))

        self.Scene = Scene
        self.PointCloud = lambda vertices, colors=None: Geometry("points", vertices=np.array(vertices), colors=np.array(colors))
        self.Trimesh = lambda vertices=None, faces=None, face_colors=None: Geometry(
            "mesh", vertices=np.array(vertices), faces=np.array(faces), face_colors=np.array(face_colors))


def _to_numpy(x):
    if isinstance(x, (list, tuple)):
        return [_to_numpy(v) for v in x]
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def _geotrf(T, pts):
    """dust3r.utils.geometry.geotrf for one 4x4 and [H, W, 3] points, in the points' precision"""
    return pts @ T[:3, :3].T + T[:3, 3]


def _pts3d_to_trimesh(img, pts3d, valid=None):
    """dust3r.viz.pts3d_to_trimesh: two triangles per pixel quad, each with its mirror, kept when all corners are valid"""
    H, W, _ = img.shape
    vertices = pts3d.reshape(-1, 3)
    idx = np.arange(len(vertices)).reshape(H, W)
    i1, i2, i3, i4 = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.concatenate((np.c_[i1, i2, i3], np.c_[i3, i2, i1], np.c_[i2, i3, i4], np.c_[i4, i3, i2]), axis=0)
    face_colors = np.concatenate((img[:-1, :-1].reshape(-1, 3), img[:-1, :-1].reshape(-1, 3), img[1:, 1:].reshape(-1, 3),
                                  img[1:, 1:].reshape(-1, 3)), axis=0)
    if valid is not None:
        keep = valid.ravel()[faces].all(axis=-1)
        faces, face_colors = faces[keep], face_colors[keep]
    return dict(vertices=vertices, face_colors=face_colors, faces=faces)


def _cat_meshes(meshes):
    n = np.cumsum([0] + [len(m["vertices"]) for m in meshes])
    return dict(vertices=np.concatenate([m["vertices"] for m in meshes]), face_colors=np.concatenate([m["face_colors"] for m in meshes]),
                faces=np.concatenate([m["faces"] + n[i] for i, m in enumerate(meshes)]))


def _reference_export(rec, cams_seen):
    from scipy.spatial.transform import Rotation
    tree = ast.parse(open(REF_GRADIO).read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("_convert_scene_output_to_glb", "get_3D_model_from_scene")]
    assert len(nodes) == 2
    for n in nodes:
        n.decorator_list = []

    def add_scene_cam(scene, pose_c2w, edge_color, image=None, focal=None, imsize=None, screen_width=0.03, **kw):
        cams_seen.append(dict(pose=np.array(pose_c2w), color=tuple(edge_color), has_image=image is not None, focal=float(focal),
                              imsize=tuple(int(v) for v in imsize), screen_width=screen_width))

    ns = dict(np=np, os=os, torch=torch, trimesh=rec, Rotation=Rotation, to_numpy=_to_numpy, geotrf=_geotrf,
              pts3d_to_trimesh=_pts3d_to_trimesh, cat_meshes=_cat_meshes, add_scene_cam=add_scene_cam, OPENGL=E.OPENGL.copy(),
              CAM_COLORS=list(E.CAM_COLORS))
    exec(compile(ast.Module(body=nodes, type_ignores=[]), REF_GRADIO, "exec"), ns)
    return ns["get_3D_model_from_scene"]


@needs_reference
@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("as_pointcloud,filename", [(True, "scene.glb"), (True, "cloud.ply"), (False, "scene.glb")])   # ply + mesh: refused, below
def test_reference_decisions_equal_host_planning(tmp_path, as_pointcloud, local, filename):
    scene = R.make_scene(SHAPES, seed=14)
    med = sorted(float(x["conf"].median()) for x in scene.x_out)
    cam_thr, thr = 0.5 * (med[1] + med[2]), 2.0
    rec, cams = _Trimesh(), []
    ref_fn = _reference_export(rec, cams)
    out = ref_fn(str(tmp_path), False, scene, min_conf_thr=thr, as_pointcloud=as_pointcloud, transparent_cams=False,
                 local_pointmaps=local, cam_size=0.07, camera_conf_thr=cam_thr, filename=filename)
    assert out == os.path.join(str(tmp_path), filename)
    log = {e[0]: e for e in rec.log}
    assert log[("export_geometry" if filename.endswith("ply") else "export_scene")][-1 if not filename.endswith("ply") else 2] == out

    # cameras: which views reach add_scene_cam, their colours and sizes
    mask = E.camera_mask(scene.x_out, cam_thr)
    assert sum(mask) == 2
    kept = [i for i, m in enumerate(mask) if m]
    assert [c["color"] for c in cams] == [E.CAM_COLORS[i % len(E.CAM_COLORS)] for i in kept]
    assert [c["imsize"] for c in cams] == [(SHAPES[i][1], SHAPES[i][0]) for i in kept]
    assert [c["focal"] for c in cams] == [scene.focals[i] for i in kept] and all(c["screen_width"] == 0.07 for c in cams)
    assert all(np.array_equal(c["pose"], scene.cams2world[i].numpy()) for c, i in zip(cams, kept))

    # the matrix
    T = log["apply_transform"][1]
    S, M = E.view_matrices(scene.cams2world, local)
    assert T.dtype == np.float64 and np.array_equal(T, S) and np.array_equal(T, R.scene_transform(scene.cams2world[0]))

    # the geometry: selection, order, colours, faces (before the transform: an identity map in the restatement)
    views = R.scene_views(scene, False)     # the reference always hands WORLD points to trimesh (fp32 geotrf of the local ones if asked)
    if local:
        views = [(c, _geotrf(x["c2w"], x["pts3d_local"]).numpy(), rgb) for (c, _, rgb), x in zip(views, scene.x_out)]
    eye = [np.eye(4)[:3]] * len(views)
    kind, kw = log["add_geometry"][1:]
    if as_pointcloud:
        pos, col = R.pointcloud(views, eye, thr)
        assert kind == "points" and kw["vertices"].dtype == np.float32
        assert np.array_equal(kw["vertices"], pos) and np.array_equal(R.quantise(kw["colors"]), col)
        ref_world = kw["vertices"]
        want = R.pointcloud(R.scene_views(scene, local), list(M), thr)[0]
    else:
        pos, col, faces = R.mesh(views, eye, thr)
        assert kind == "mesh" and np.array_equal(kw["vertices"], pos) and np.array_equal(kw["faces"], faces.astype(np.int64))
        assert len(faces) > 0
        ref_world = kw["vertices"]
        want = R.mesh(R.scene_views(scene, local), list(M), thr)[0]

    # positions after the transform: the reference's route (trimesh applies T in fp64 to the fp32 points) rounded once to fp32
    ref_final = R.transform(T[:3], ref_world)
    if not local:
        assert np.array_equal(ref_final.view(np.uint32), want.view(np.uint32))
        return
    # local_pointmaps: the reference rounds to fp32 after geotrf, the design does not: the bound of that one extra rounding, in fp64
    u = 2.0 ** -24
    if as_pointcloud:
        sel = [R.select(x["conf"], thr) for x in scene.x_out]
    else:
        sel = [np.ones(s, dtype=bool) for s in SHAPES]
    bound = []
    for x, m in zip(scene.x_out, sel):
        c = x["c2w"].double().numpy()
        p = np.abs(x["pts3d_local"].double().numpy()[m])
        e1 = 4 * u * (p @ np.abs(c[:3, :3]).T + np.abs(c[:3, 3]))
        bound.append(e1 @ np.abs(S[:3, :3]).T)
    bound = np.concatenate(bound) + 2 * u * np.abs(want.astype(np.float64))
    err = np.abs(ref_final.astype(np.float64) - want.astype(np.float64))
    print("local_pointmaps: max err / bound =", float((err / bound).max()))
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals and the CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ply_mesh_is_refused_and_none_scene(tmp_path):
    scene = R.make_scene([(6, 8)], seed=15)
    with pytest.raises(ValueError, match="ply"):
        Dm.get_3D_model_from_scene(str(tmp_path), False, scene, as_pointcloud=False, filename="scene.ply")
    assert os.listdir(tmp_path) == []
    assert Dm.get_3D_model_from_scene(str(tmp_path), False, None) is None
    assert Dm.export_scene_thresholds(str(tmp_path), None, [3.0]) == []
    with pytest.raises(ValueError):
        Dm.export_scene_thresholds(str(tmp_path), scene, [3.0], file_type="obj")


def test_signature_is_the_references():
    import inspect
    sig = inspect.signature(Dm.get_3D_model_from_scene)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("outdir", inspect.Parameter.empty), ("verbose", inspect.Parameter.empty), ("scene", inspect.Parameter.empty),
        ("min_conf_thr", 3.0), ("as_pointcloud", False), ("transparent_cams", False), ("local_pointmaps", False), ("cam_size", 0.05),
        ("camera_conf_thr", 0.0), ("filename", "scene.glb")]


def _parser_table(parser):
    out = {}
    for a in parser._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        out[tuple(a.option_strings)] = dict(dest=a.dest, default=a.default, choices=None if a.choices is None else list(a.choices),
                                            required=a.required, type=a.type, nargs=a.nargs, const=a.const, kind=type(a).__name__)
    return out


@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="the reference checkout is not present")
def test_cli_parser_equals_reference():
    from must3r_amd.model import MEMORY_MODES
    tree = ast.parse(open(REF_CLI).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_args_parser")
    ns = dict(argparse=argparse, MEMORY_MODES=MEMORY_MODES)
    exec(compile(ast.Module(body=[node], type_ignores=[]), REF_CLI, "exec"), ns)
    ref, nat = _parser_table(ns["get_args_parser"]()), _parser_table(G.get_args_parser())
    assert list(ref) == list(nat)
    assert ref == nat
    assert nat[("--file_type",)]["choices"] == ["glb", "ply"] and E.REFERENCE_THRESHOLDS == (6.0, 5.0, 4.0, 3.0, 2.5, 2.0, 1.5, 1.05)
