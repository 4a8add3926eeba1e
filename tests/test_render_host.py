"""Host side of the scene renderer (must3r_amd.render, csrc/render.hip's descriptor checks, the numpy restatement tests/render_ref.py), no GPU
needed: the ABI surface and the descriptor layouts, every refusal (each returns before anything is uploaded or launched), the camera planners
against their formulas, and the restatement itself on a scene small enough to work out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import export_ref as R
import render_ref as RR
from conftest import ROOT
from must3r_amd import _lib, render as Rn, slam


def _header():
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------------------------
# ABI and layout
# ---------------------------------------------------------------------------------------------------------------------------------
_CTYPE = {"int32_t": 4, "float": 4, "double": 8, "size_t": 8, "uint8_t": 1}


def _struct_layout(name):
    """(field, offset) of a descriptor as the header declares it, by the C rules for the x86-64 ABI; arrays count as their element"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, out, widest = 0, [], 1
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl, flags=re.S)
        size = 8 if m.group(2) else _CTYPE[m.group(1)]
        widest = max(widest, size)
        for field in (f.strip() for f in m.group(3).split(",")):
            count = 1
            arr = re.match(r"(\w+)\[(\d+)\]$", field)
            if arr:
                field, count = arr.group(1), int(arr.group(2))
            off = (off + size - 1) // size * size
            out.append((field, off))
            off += size * count
    return out, (off + widest - 1) // widest * widest


@pytest.mark.parametrize("cname,cls", [("must3r_hip_render_camera", "RenderCamera"), ("must3r_hip_render_desc", "RenderDesc")])
def test_descriptor_offsets_match_the_header(cname, cls):
    st = getattr(_lib, cls)
    layout, size = _struct_layout(cname)
    assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == layout
    assert C.sizeof(st) == size
    assert C.sizeof(_lib.RenderCamera) == 144 and _lib.RenderDesc.scratch.offset == 40


def _align(x):
    return (x + 255) // 256 * 256


def _scratch(nv, nc, W, H):
    return _align(40 * nv) + _align(40 * nc) + _align(96 * nc * nv) + _align(8 * nc * W * H)


def _desc(n_views=2, n_cams=2, W=64, H=48, vh=12, vw=16, ptr=None):
    """a valid descriptor over host addresses that are never read; returns it with the objects it points to"""
    buf = (C.c_double * 64)()
    p = C.addressof(buf) if ptr is None else ptr
    views = (_lib.ExportView * max(n_views, 1))()
    for e in views:
        e.conf = e.pts = e.rgb = p
        e.H, e.W = vh, vw
    cams = (_lib.RenderCamera * max(n_cams, 1))()
    for e in cams:
        e.fx = e.fy = 10.0
        e.z_near, e.z_far, e.W, e.H = 0.01, 100.0, W, H
    d = _lib.RenderDesc()
    d.views, d.cams, d.n_views, d.n_cams, d.thr, d.point_size = views, cams, n_views, n_cams, 1.5, 1
    d.scratch, d.scratch_bytes = p // 256 * 256 + 256, 1 << 40
    d.rgb = d.depth = d.index = p
    return d, (buf, views, cams)


def test_abi_surface_and_scratch_bytes():
    h = _header()
    assert _lib.ABI_VERSION == 21 and re.search(r"#define\s+MUST3R_HIP_ABI_VERSION\s+21\b", h)
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == 21
    assert "ABI 21, additive: scene rendering" in h
    for name, proto in (("must3r_hip_render_scratch_bytes", (C.c_size_t, [C.POINTER(_lib.RenderDesc)])),
                        ("must3r_hip_render", (C.c_int, [C.POINTER(_lib.RenderDesc)]))):
        assert name in _lib.EXPORTS and _lib.PROTOTYPES[name] == proto and hasattr(lib, name)
    assert re.search(r"\bsize_t\s+must3r_hip_render_scratch_bytes\s*\(\s*const\s+must3r_hip_render_desc\s*\*\s*d\s*\)\s*;", h)
    assert re.search(r"\bint\s+must3r_hip_render\s*\(\s*const\s+must3r_hip_render_desc\s*\*\s*d\s*\)\s*;", h)
    assert int(re.search(r"#define\s+MUST3R_RENDER_MAX_POINT_SIZE\s+(\d+)", h).group(1)) == _lib.RENDER_MAX_POINT_SIZE == 8
    with open(os.path.join(ROOT, "must3r_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS\s*=.*\brender\.hip\b", mk, flags=re.M) and re.search(r"^build/render\.o: FLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    # the stated sizes: four sections, each rounded up to 256 bytes
    d, keep = _desc(n_views=5, n_cams=2, W=64, H=48)
    assert lib.must3r_hip_render_scratch_bytes(C.byref(d)) == _scratch(5, 2, 64, 48) == 256 + 256 + 1024 + 49152
    d, keep = _desc(n_views=200, n_cams=120, W=512, H=384, vh=384, vw=512)
    assert lib.must3r_hip_render_scratch_bytes(C.byref(d)) == _scratch(200, 120, 512, 384) == 8192 + 4864 + 2304000 + 188743680
    assert lib.must3r_hip_render_scratch_bytes(None) == 0 and "null" in lib.must3r_hip_last_error().decode()


def _refused(d, word):
    lib = _lib.load()
    assert lib.must3r_hip_render(C.byref(d)) != 0
    msg = lib.must3r_hip_last_error().decode()
    assert word in msg, (word, msg)


def test_refusals_before_any_launch():
    """every refusal the header lists; the pointers are host addresses, so a call that got as far as an upload or a launch would not return cleanly"""
    lib = _lib.load()
    assert lib.must3r_hip_render(None) != 0 and "null descriptor" in lib.must3r_hip_last_error().decode()
    for ps in (0, 9, -1):
        d, keep = _desc()
        d.point_size = ps
        _refused(d, "point_size")
        assert lib.must3r_hip_render_scratch_bytes(C.byref(d)) == 0
    for field in ("W", "H"):
        d, keep = _desc()
        for e in keep[2]:
            setattr(e, field, 0)
        _refused(d, "non-positive image size")
    d, keep = _desc(); d.n_cams = 0; _refused(d, "camera table is empty")
    d, keep = _desc(); d.n_views = 0; _refused(d, "view table is empty")
    d, keep = _desc(); keep[2][1].W = 65; _refused(d, "share one image size")
    d, keep = _desc(); keep[2][1].H = 47; _refused(d, "share one image size")
    d, keep = _desc(); d.views = None; _refused(d, "null view table")
    d, keep = _desc(); d.cams = None; _refused(d, "null camera table")
    d, keep = _desc(); keep[1][1].H = 0; _refused(d, "a view has a non-positive size")
    for zn, zf in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.1, float("inf")), (0.1, float("nan"))):
        d, keep = _desc()
        keep[2][0].z_near, keep[2][0].z_far = zn, zf
        _refused(d, "z_near")
    # 2^32 source pixels, 2^31 in one view, 2^31 target pixels: arithmetic on the sizes alone
    d, keep = _desc(n_views=3, vh=32768, vw=43691)
    assert 3 * 32768 * 43691 >= 2 ** 32 > 2 * 32768 * 43691
    _refused(d, "2^32")
    d.n_views = 2
    assert lib.must3r_hip_render_scratch_bytes(C.byref(d)) > 0
    d, keep = _desc(n_views=1, vh=65536, vw=32768); _refused(d, "2^31")
    d, keep = _desc(n_cams=2, W=32768, H=32768); _refused(d, "target pixels")
    # the scratch
    d, keep = _desc(); d.scratch = None; _refused(d, "null scratch")
    d, keep = _desc(); d.scratch_bytes = _scratch(2, 2, 64, 48) - 1; _refused(d, "scratch too small")
    d, keep = _desc(); d.scratch += 8; _refused(d, "aligned")
    for plane in ("conf", "pts", "rgb"):
        d, keep = _desc()
        setattr(keep[1][1], plane, None)
        _refused(d, "null plane")


def test_python_wrapper_refusals():
    with pytest.raises(SystemExit, match="--render_dir"):
        slam.main(["--chkpt", "x", "--input", "y", "--gui"])
    a = slam.get_parser().parse_args(["--chkpt", "x"])
    assert a.render_dir is None
    from must3r_amd import get_reconstruction as G
    a = G.get_cli_parser().parse_args(["--image_dir", "i", "--output", "o"])
    assert a.render_dir is None and a.render_views == 0
    import inspect
    from must3r_amd import demo
    sig = inspect.signature(demo.get_reconstructed_scene).parameters
    assert sig["render_dir"].default is None and sig["render_views"].default == 0 and list(sig)[-2:] == ["render_dir", "render_views"]
    sig = inspect.signature(Rn.render_scene).parameters
    assert [(k, sig[k].default) for k in ("thr", "point_size", "local_pointmaps", "depth")] == [("thr", 3.0), ("point_size", 2), ("local_pointmaps", False),
                                                                                                 ("depth", False)]


# ---------------------------------------------------------------------------------------------------------------------------------
# camera planning
# ---------------------------------------------------------------------------------------------------------------------------------
def _pose(seed):
    g = np.random.default_rng(seed)
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = q, g.standard_normal(3)
    return c2w


def _project(cam, p):
    X = np.asarray(cam.w2c) @ np.append(np.asarray(p, dtype=np.float64), 1.0)
    return cam.fx * X[0] / X[2] + cam.cx, cam.fy * X[1] / X[2] + cam.cy, X[2]


def _same_camera(a, b, atol=1e-12):
    assert np.allclose(np.asarray(a.w2c), np.asarray(b.w2c), rtol=0, atol=atol)
    assert np.allclose([a.fx, a.fy, a.cx, a.cy], [b.fx, b.fy, b.cx, b.cy], rtol=1e-15, atol=0) and (a.W, a.H) == (b.W, b.H)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_look_at_and_follow_camera(seed):
    c2w = _pose(seed)
    W, H = 96, 64
    cam = Rn.follow_camera(torch.from_numpy(c2w).float(), W, H)
    c2w = c2w.astype(np.float32).astype(np.float64)
    _same_camera(cam, RR.follow_camera(c2w, W, H))
    Rw = np.asarray(cam.w2c)[:, :3]
    assert np.allclose(Rw @ Rw.T, np.eye(3), rtol=0, atol=1e-14) and abs(np.linalg.det(Rw) - 1) < 1e-14
    assert cam.fx == cam.fy == (H / 2) / np.tan(np.deg2rad(60.0) / 2) and (cam.cx, cam.cy) == (W / 2, H / 2)
    # the looked-at centre lands on the principal point, sqrt(.6^2 + 1.5^2) in front; the eye is the camera's origin
    u, v, z = _project(cam, c2w[:3, 3])
    assert abs(u - cam.cx) < 1e-9 and abs(v - cam.cy) < 1e-9 and abs(z - np.hypot(.6, 1.5)) < 1e-6
    eye = c2w[:3, 3] + c2w[:3, :3] @ np.array([0, -.6, -1.5])
    assert np.allclose(np.asarray(cam.w2c) @ np.append(eye, 1.0), 0, atol=1e-6)
    # image up is the view's up: a point above the centre (the view's -y) lands above the principal point
    _, v_up, _ = _project(cam, c2w[:3, 3] - 0.1 * c2w[:3, 1])
    assert v_up < cam.cy
    g = np.random.default_rng(10 + seed)
    center, eye, up = g.standard_normal(3), g.standard_normal(3) + 3.0, g.standard_normal(3)
    a = Rn.look_at(center, eye, up, W, H, vfov=45.0)
    _same_camera(a, RR.look_at(center, eye, up, W, H, vfov=45.0))
    Rw = np.asarray(a.w2c)[:, :3]
    assert np.allclose(Rw @ Rw.T, np.eye(3), rtol=0, atol=1e-14) and abs(np.linalg.det(Rw) - 1) < 1e-14
    u, v, z = _project(a, center)
    assert abs(u - a.cx) < 1e-9 and abs(v - a.cy) < 1e-9 and abs(z - np.linalg.norm(center - eye)) < 1e-12
    assert a.fx == (H / 2) / np.tan(np.deg2rad(45.0) / 2)


def test_view_camera():
    scene = R.make_scene([(12, 16), (9, 16)], seed=3)
    for i in (0, 1):
        cam = Rn.view_camera(scene, i)
        _same_camera(cam, RR.view_camera(scene, i))
        H, W = scene.imgs[i].shape[:2]
        assert (cam.W, cam.H, cam.cx, cam.cy, cam.fx, cam.fy) == (W, H, W / 2, H / 2, scene.focals[i], scene.focals[i])
        assert np.allclose(np.asarray(cam.w2c) @ np.append(scene.cams2world[i][:3, 3].double().numpy(), 1.0), 0, atol=1e-6)


@pytest.mark.parametrize("W,H", [(64, 48), (48, 64)])
def test_orbit_box_sees_the_whole_box(W, H):
    mn, mx = np.array([-1.0, -0.5, 2.0]), np.array([0.5, 1.5, 3.0])
    corners = np.array([[x, y, z] for x in (mn[0], mx[0]) for y in (mn[1], mx[1]) for z in (mn[2], mx[2])])
    c2w0 = _pose(7)
    cams = Rn.orbit_box(mn, mx, c2w0, 12, W, H, vfov=60.0, elevation_deg=20.0)
    assert len(cams) == 12
    eyes = []
    for cam in cams:
        Rw = np.asarray(cam.w2c)[:, :3]
        assert np.allclose(Rw @ Rw.T, np.eye(3), rtol=0, atol=1e-14) and (cam.W, cam.H) == (W, H)
        for p in corners:
            u, v, z = _project(cam, p)
            assert np.float32(cam.z_near) <= z <= np.float32(cam.z_far) and 0 <= u < W and 0 <= v < H, (u, v, z)
        u, v, _ = _project(cam, 0.5 * (mn + mx))
        assert abs(u - cam.cx) < 1e-9 and abs(v - cam.cy) < 1e-9
        eyes.append(-Rw.T @ np.asarray(cam.w2c)[:, 3])
    eyes = np.array(eyes)
    # a circle about the axis (view 0's up direction): equal heights along it, equal distances from the centre, all eyes different
    axis = -c2w0[:3, 1]
    rel = eyes - 0.5 * (mn + mx)
    assert np.allclose(rel @ axis, (rel @ axis)[0], atol=1e-12) and (rel @ axis)[0] > 0
    assert np.allclose(np.linalg.norm(rel, axis=1), np.linalg.norm(rel[0]), atol=1e-12)
    assert min(np.linalg.norm(eyes[i] - eyes[j]) for i in range(12) for j in range(i)) > 0.1


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement, by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def _three_points():
    """camera at the identity, fx = fy = 10, cx = cy = 2, a 4 x 4 image.  P0 (0, 0, 1): u = v = 2.  P1 (-0.23, 0, 1): u = -0.3 (fp32 -0.23 is a little
    below: u = -0.30000000447), v = 2.  P2 (0, 0, 2): u = v = 2, behind P0."""
    pts = np.array([[[0, 0, 1], [-0.23, 0, 1], [0, 0, 2]]], dtype=np.float32)
    conf = np.array([[2.0, 2.0, 2.0]], dtype=np.float32)
    rgb = np.array([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]], dtype=np.float32)
    cam = RR.Camera(np.eye(4)[:3], 10.0, 10.0, 2.0, 2.0, 4, 4, 0.01, 100.0)
    return [(conf, pts, rgb)], cam


def test_restatement_by_hand():
    views, cam = _three_points()
    E = 0xFFFFFFFF
    rgb, depth, index = RR.render(views, RR.identity(1), cam, 1.5, point_size=1, background=(9, 8, 7))
    want = np.full((4, 4), E, dtype=np.uint32)
    want[2, 2] = 0                        # P0 in front of P2; P1's column floor(-0.3) = -1 is off the image (a truncating cast would say column 0)
    assert np.array_equal(index, want) and index[2, 0] == E
    assert depth[2, 2] == 1.0 and np.isposinf(depth[want == E]).all()
    assert rgb[2, 2].tolist() == [255, 0, 128] and (rgb[want == E] == [9, 8, 7]).all()      # rint(127.5) = 128: to nearest even
    # point_size 2: first column floor(u - 0.5).  P0, P2: columns and rows 1, 2.  P1: columns floor(-0.8) = -1 and 0, rows 1, 2: column 0 is left
    rgb, depth, index = RR.render(views, RR.identity(1), cam, 1.5, point_size=2)
    want = np.full((4, 4), E, dtype=np.uint32)
    want[1:3, 1:3] = 0
    want[1:3, 0] = 1
    assert np.array_equal(index, want) and (depth[want != E] == 1.0).all() and rgb[1, 0].tolist() == [0, 255, 0]
    # a threshold between: P0 alone dropped -> P2 shows with depth 2; NaN confidence never passes
    views[0][0][0, 0] = 1.0
    views[0][0][0, 1] = np.nan
    _, depth, index = RR.render(views, RR.identity(1), cam, 1.5)
    assert index[2, 2] == 2 and depth[2, 2] == 2.0 and (index != E).sum() == 1
    # a tie in depth goes to the lower index; z exactly at z_near / z_far is kept, one ulp outside is not
    views, cam = _three_points()
    views[0][1][0, 2] = [0, 0, 1]
    assert RR.render(views, RR.identity(1), cam, 1.5)[2][2, 2] == 0
    for z, kept in ((np.float32(0.01), True), (np.nextafter(np.float32(0.01), np.float32(0)), False), (np.float32(100.0), True),
                    (np.nextafter(np.float32(100.0), np.float32(200)), False)):
        views[0][1][0] = [[0, 0, z]] * 3
        _, depth, index = RR.render(views, RR.identity(1), cam, 1.5)
        assert (index[2, 2] == 0 and depth[2, 2] == z) if kept else (index == E).all(), z


def test_restatement_composition_and_matrices():
    """the composed matrix against numpy's product; a view matrix moves the points as the export's transform does"""
    g = np.random.default_rng(0)
    w2c, M = g.standard_normal((3, 4)), g.standard_normal((3, 4))
    full = lambda m: np.vstack([m, [0, 0, 0, 1]])   # noqa: E731
    assert np.allclose(RR.compose(w2c, M), (full(w2c) @ full(M))[:3], rtol=1e-14, atol=1e-14)
    assert np.array_equal(RR.compose(np.eye(4)[:3], M), M) and np.array_equal(RR.compose(w2c, np.eye(4)[:3]), w2c)
    views, cam = _three_points()
    shift = np.eye(4)[:3].copy()
    shift[0, 3] = 0.1                     # one pixel to the right at depth 1, half a pixel at depth 2: P2 (u = 2.5) is no longer hidden
    index = RR.render(views, [shift], cam, 1.5)[2]
    assert index[2, 3] == 0 and index[2, 0] == 1 and index[2, 2] == 2 and (index != 0xFFFFFFFF).sum() == 3
