"""The input cases of the mesh rasteriser's tests (tests/test_render_mesh_host.py on the CPU, tests/test_render_mesh_gpu.py on the device): small
coherent surfaces, so that the triangles mean something, and cameras chosen so that every part of the rule is exercised.  Each builder returns
(views, matrices, cameras, thr) with views a list of (conf [H, W], pts [H, W, 3], rgb [H, W, 3]) fp32 numpy arrays; ``want`` computes the
restatement's answer once per case and camera and keeps it."""
import numpy as np

import render_mesh_ref as MR
import render_ref as RR

THR = 1.5
_cache = {}


def surface(H, W, x0, x1, y0, y1, z, seed, tilt=0.0, wave=0.05):
    """a smooth height field over [x0, x1] x [y0, y1]: z + tilt x + wave sin(3 x) cos(2 y); confidence 2, smooth colours a little outside [0, 1]"""
    r, c = np.mgrid[0:H, 0:W]
    x = x0 + (x1 - x0) * c / max(W - 1, 1)
    y = y0 + (y1 - y0) * r / max(H - 1, 1)
    pts = np.stack([x, y, z + tilt * x + wave * np.sin(3 * x + seed) * np.cos(2 * y)], axis=-1).astype(np.float32)
    conf = np.full((H, W), 2.0, dtype=np.float32)
    rgb = np.stack([0.5 + 0.6 * np.sin(x + seed), 0.5 + 0.6 * np.cos(2 * y), 0.5 + 0.3 * np.sin(x * y + seed)], axis=-1).astype(np.float32)
    return conf, pts, rgb


def _rot_y(a, t):
    M = np.eye(4)[:3].copy()
    M[0, 0], M[0, 2], M[2, 0], M[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    M[:, 3] = t
    return M


def cam(fx, fy, cx, cy, W, H, z_near=0.01, z_far=100.0, w2c=None):
    return RR.Camera(np.eye(4)[:3] if w2c is None else np.asarray(w2c, dtype=np.float64), float(fx), float(fy), float(cx), float(cy), W, H, z_near, z_far)


def main_case():
    """four views (9 x 13, 16 x 16, 2 x 2 and a 1 x 7 strip without a triangle) under non-identity matrices, three cameras of 40 x 30"""
    v0 = surface(9, 13, -1.3, 1.2, -0.9, 0.8, 2.0, 0)
    v1 = surface(16, 16, -0.9, 1.5, -1.0, 0.9, 2.5, 1, tilt=0.25)
    v2 = surface(2, 2, -2.5, 0.4, -1.8, 0.3, 3.2, 2, tilt=-0.1)
    v3 = surface(1, 7, -1.0, 1.0, 0.0, 0.0, 1.5, 3)
    views = [v0, v1, v2, v3]
    # confidences that remove single corners, NaN and inf points
    v0[0][2, 3] = 1.0
    v0[0][5, 9] = np.nan
    v1[0][7, 7] = 1.49
    v1[0][0, 15] = -np.inf
    v0[1][4, 6, 2] = np.nan
    v1[1][10, 3, 0] = np.inf
    v1[1][12, 12, 1] = -np.inf
    v1[1][3, 11] = [0.9, -0.6, 0.004]              # in front of the eye and behind every near plane
    matrices = [_rot_y(0.05, [0.02, -0.01, 0.0]), _rot_y(-0.12, [0.1, 0.05, 0.1]), _rot_y(0.2, [0.0, 0.0, -0.2]), np.eye(4)[:3]]
    w2c1 = _rot_y(0.35, [0.3, 0.1, -0.9])            # closer and oblique: larger triangles, part of the scene off the image
    w2c2 = _rot_y(-0.2, [-0.6, -0.2, 0.1])
    cams = [cam(26.0, 25.0, 20.0, 15.0, 40, 30), cam(22.0, 21.0, 18.0, 14.0, 40, 30, z_near=1.25, w2c=w2c1),
            cam(27.0, 26.0, 26.0, 16.0, 40, 30, z_far=2.55, w2c=w2c2)]
    return views, matrices, cams, THR


def lattice_case():
    """vertices, outline edges and diagonals on sample points: fx = fy = 1, cx = cy = 0, z = 1, a 4 x 4 grid of vertices at 0.5 + 2 k in an 8 x 8 image.
    The pixel centres with both coordinates in [0.5, 6.5] are the 49 that lie inside or on the outline."""
    k = 0.5 + 2.0 * np.arange(4)
    x, y = np.meshgrid(k, k)
    pts = np.stack([x, y, np.ones_like(x)], axis=-1).astype(np.float32)
    rgb = np.stack([x / 7, y / 7, 0.5 * np.ones_like(x)], axis=-1).astype(np.float32)
    return [(np.full((4, 4), 2.0, dtype=np.float32), pts, rgb)], RR.identity(1), [cam(1.0, 1.0, 0.0, 0.0, 8, 8)], THR


def plane_case():
    """a planar 12 x 12 grid seen obliquely from a close camera: a triangle covers many of the 64 x 48 target pixels"""
    conf, pts, rgb = surface(12, 12, -1.0, 1.0, -1.0, 1.0, 0.0, 4, wave=0.0)
    w2c = _rot_y(0.0, [0.0, 0.0, 0.0])
    a = 0.9                                           # the plane z = 0 tilted about the x axis and pushed away
    w2c[1, 1], w2c[1, 2], w2c[2, 1], w2c[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    w2c[:, 3] = [0.1, 0.25, 1.6]
    return [(conf, pts, rgb)], RR.identity(1), [cam(40.0, 40.0, 32.0, 24.0, 64, 48, w2c=w2c)], THR


def plane_outline(views, matrices, camera):
    """the projected corners of the plane case's grid, in order around the outline -> fp64 [4, 2]"""
    pts = views[0][1]
    corners = np.stack([pts[0, 0], pts[0, -1], pts[-1, -1], pts[-1, 0]])
    _, u, v = RR.project(RR.compose(camera.w2c, matrices[0]), camera, corners)
    return np.stack([u, v], axis=1)


def inside_outline(outline, W, H, margin):
    """bool [H, W]: the pixel centres at least `margin` pixels inside the convex quadrilateral `outline`"""
    q, r = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ok = np.ones((H, W), dtype=bool)
    sign = None
    for k in range(4):
        a, b = outline[k], outline[(k + 1) % 4]
        n = np.array([-(b[1] - a[1]), b[0] - a[0]]) / np.hypot(*(b - a))
        d = (q - a[0]) * n[0] + (r - a[1]) * n[1]
        if sign is None:
            c = outline.mean(axis=0)
            sign = np.sign((c[0] - a[0]) * n[0] + (c[1] - a[1]) * n[1])
        ok &= sign * d >= margin
    return ok


def sizes_case(wave_area):
    """one quad (0.4, 0.4) .. (1.4, 1.4) at z = 1 and cameras whose focal lengths give its triangles candidate boxes of wave_area - 1, wave_area and
    wave_area + 1 pixels, then one from so close that triangle 0 covers the whole 16 x 16 target"""
    assert wave_area == 64, "the box shapes below are chosen for 64"
    xy = np.array([[[0.4, 0.4], [1.4, 0.4]], [[0.4, 1.4], [1.4, 1.4]]])
    pts = np.concatenate([xy, np.ones((2, 2, 1))], axis=-1).astype(np.float32)
    rgb = np.array([[[1.0, 0, 0], [0, 1.0, 0]], [[0, 0, 1.0], [1.0, 1.0, 0]]], dtype=np.float32)
    cams = [cam(fx, fy, 0.4 - 0.4 * fx, 0.4 - 0.4 * fy, 16, 16) for fx, fy in ((7, 9), (8, 8), (5, 13))]
    cams.append(cam(200.0, 200.0, -10.0 - 0.4 * 200, -10.0 - 0.4 * 200, 16, 16))
    return [(np.full((2, 2), 2.0, dtype=np.float32), pts, rgb)], RR.identity(1), cams, THR


def degenerate_case():
    """view 0: a = b (two equal corners) and b, c', d collinear: den == 0 in both triangles.  View 1: a corner at u = v = 3e300 through a matrix that scales
    x and y by 1e262: the edge products overflow, den is not finite.  Every triangle has candidates; none covers a pixel."""
    p0 = np.array([[[1, 1, 1], [1, 1, 1]], [[3, 3, 1], [5, 5, 1]]], dtype=np.float32)
    p1 = np.array([[[3e38, 3e38, 1], [0, 0, 1]], [[0, 0, 1], [0, 0, 1]]], dtype=np.float32)
    M1 = np.eye(4)[:3].copy()
    M1[0, 0] = M1[1, 1] = 1e262
    M1[0, 3], M1[1, 3] = 2.0, 3.0
    conf = np.full((2, 2), 2.0, dtype=np.float32)
    rgb = np.full((2, 2, 3), 0.5, dtype=np.float32)
    return [(conf, p0, rgb), (conf.copy(), p1, rgb.copy())], [np.eye(4)[:3], M1], [cam(1.0, 1.0, 0.0, 0.0, 8, 8)], THR


def twin_case():
    """two coincident views with different colours: equal fp32 depth everywhere"""
    a = surface(6, 7, -1.0, 1.0, -0.8, 0.8, 2.0, 5, tilt=0.1)
    b = (a[0].copy(), a[1].copy(), (1.0 - a[2]).astype(np.float32))
    return [a, b], RR.identity(2), [cam(12.0, 12.0, 16.0, 12.0, 32, 24)], THR


def blocks_case():
    """a 37 x 40 view (1480 pixels: two source blocks, rows that straddle the threads' groups of four and the block boundary) over a 33 x 37 one, seen from
    two cameras of 48 x 36, the second close enough that many triangles of one wave take the wave path"""
    v0 = surface(37, 40, -1.2, 1.2, -0.9, 0.9, 2.0, 6, tilt=0.15, wave=0.08)
    v1 = surface(33, 37, -1.0, 1.3, -1.0, 0.8, 2.3, 7, tilt=-0.2, wave=0.1)
    v0[0][::7, ::5] = 1.0
    v1[1][5::9, 3::8, 2] = np.nan
    matrices = [_rot_y(0.03, [0.0, 0.02, 0.0]), _rot_y(-0.08, [0.05, 0.0, 0.05])]
    cams = [cam(36.0, 36.0, 24.0, 18.0, 48, 36), cam(420.0, 420.0, 30.0, 10.0, 48, 36, w2c=_rot_y(0.1, [0.1, 0.0, -0.3]))]
    return [v0, v1], matrices, cams, THR


def want(name, builder, ci, **defects):
    """the restatement's (rgb, depth, index, contenders) of camera `ci` of a case, computed once and left unchanged"""
    key = (name, ci, tuple(sorted(defects.items())))
    if key not in _cache:
        views, matrices, cams, thr = case(name, builder)
        _cache[key] = MR.render(views, matrices, cams[ci], thr, **defects)
    return _cache[key]


def case(name, builder):
    if ("case", name) not in _cache:
        _cache[("case", name)] = builder()
    return _cache[("case", name)]
