"""numpy restatement of the scene renderer (what must3r_amd.render / csrc/render.hip must produce), written from the description of the
method in include/must3r_hip.h, not from the kernels:

  composition  A = w2c . M per (camera, view), fp64, explicit scalar loops: per element the three products summed in ascending k, then (last
               column) the translation added
  projection   per source pixel (x, y, z) fp32 and camera, fp64 numpy ufuncs one by one (numpy does not fuse):
               X_a = ((A[a][0] x + A[a][1] y) + A[a][2] z) + A[a][3];  Z = X_2;  u = fx (X_0 (1.0 / Z)) + cx;  v = fy (X_1 (1.0 / Z)) + cy
  drop         conf >= fp32(thr) fails | x, y, z, u, v not finite | not (z_near <= Z <= z_far)      -- before any conversion to an integer
  cover        the square of point_size pixels from column floor(u - (point_size - 1) / 2), row floor(v - (point_size - 1) / 2), clipped
  z-buffer     np.minimum.at over uint64 keys (bits(fp32 Z) << 32) | global source index (views in order, pixels row-major)
  resolve      empty -> background, +inf, 0xFFFFFFFF; else the key's fp32 depth, its index and export_ref.quantise of that pixel's colour
and the camera planners from their formulas.
"""
import collections

import numpy as np

from export_ref import np32, np64, quantise, select

Camera = collections.namedtuple("Camera", "w2c fx fy cx cy W H z_near z_far")
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def compose(w2c, M):
    """3x4 . 3x4 (implied last row 0 0 0 1) with explicit scalar loops"""
    w2c, M = np64(w2c).reshape(3, 4), np64(M).reshape(3, 4)
    A = np.zeros((3, 4), dtype=np.float64)
    for a in range(3):
        for b in range(4):
            s = w2c[a, 0] * M[0, b]
            s = s + w2c[a, 1] * M[1, b]
            s = s + w2c[a, 2] * M[2, b]
            if b == 3:
                s = s + w2c[a, 3]
            A[a, b] = s
    return A


def project(A, cam, pts):
    """pts fp32 [n, 3] -> (Z, u, v) fp64 [n]"""
    p = np32(pts).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        X = [((A[a, 0] * x + A[a, 1] * y) + A[a, 2] * z) + A[a, 3] for a in range(3)]
        Z = X[2]
        iz = 1.0 / Z
        u = np.float64(cam.fx) * (X[0] * iz) + np.float64(cam.cx)
        v = np.float64(cam.fy) * (X[1] * iz) + np.float64(cam.cy)
    return Z, u, v


def contenders(views, matrices, cam, thr, point_size=1):
    """-> (target pixel int64 [m], key uint64 [m], stats): every (covered target pixel, key) pair of one camera before the minimum.
    stats: selected points, of them behind the camera's near plane (Z < z_near), and in front, inside the depth range and outside the image (point_size 1)"""
    half = np.float64(0.5 * (point_size - 1))
    W, H = int(cam.W), int(cam.H)
    zn, zf = np.float64(np.float32(cam.z_near)), np.float64(np.float32(cam.z_far))
    pix, keys, base = [], [], 0
    stats = dict(selected=0, behind=0, outside=0)
    for (conf, pts, _), M in zip(views, matrices):
        conf, pts = np32(conf).reshape(-1), np32(pts).reshape(-1, 3)
        A = compose(cam.w2c, M)
        Z, u, v = project(A, cam, pts)
        sel = select(conf, thr)
        with np.errstate(all="ignore"):
            keep = sel & np.isfinite(pts).all(axis=1) & np.isfinite(u) & np.isfinite(v) & (Z >= zn) & (Z <= zf)
            c0, r0 = np.floor(u - half), np.floor(v - half)
            keep &= (c0 < W) & (c0 + point_size > 0) & (r0 < H) & (r0 + point_size > 0)
            stats["selected"] += int(sel.sum())
            stats["behind"] += int((sel & (Z < zn)).sum())
            inside = (np.floor(u) >= 0) & (np.floor(u) < W) & (np.floor(v) >= 0) & (np.floor(v) < H)
            stats["outside"] += int((sel & (Z >= zn) & (Z <= zf) & np.isfinite(u) & np.isfinite(v) & ~inside).sum())
        idx = np.nonzero(keep)[0]
        c0, r0 = c0[idx].astype(np.int64), r0[idx].astype(np.int64)        # inside (-point_size, W) resp. (-point_size, H): safe to convert
        key = (Z[idx].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx + base).astype(np.uint64)
        for dr in range(point_size):
            for dc in range(point_size):
                r, c = r0 + dr, c0 + dc
                ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
                pix.append(r[ok] * W + c[ok])
                keys.append(key[ok])
        base += conf.size
    return np.concatenate(pix), np.concatenate(keys), stats


def render(views, matrices, cam, thr, point_size=1, background=(255, 255, 255)):
    """views: list of (conf [H, W], pts [H, W, 3], rgb [H, W, 3]) -> rgb uint8 [H, W, 3], depth fp32 [H, W], index uint32 [H, W] of one camera"""
    W, H = int(cam.W), int(cam.H)
    pix, keys, _ = contenders(views, matrices, cam, thr, point_size)
    zbuf = np.full(H * W, EMPTY, dtype=np.uint64)
    np.minimum.at(zbuf, pix, keys)
    hit = zbuf != EMPTY
    index = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    depth = (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    depth[~hit] = np.inf
    colours = np.concatenate([quantise(np32(rgb).reshape(-1, 3))[:, :3] for _, _, rgb in views])
    rgb = np.empty((H * W, 3), dtype=np.uint8)
    rgb[:] = np.asarray(background, dtype=np.uint8)
    rgb[hit] = colours[index[hit]]
    return rgb.reshape(H, W, 3), depth.reshape(H, W), index.reshape(H, W)


def identity(n):
    return [np.eye(4)[:3] for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------------------------
# camera planning
# ------------------------------------------------------------------------------------------------------------------------------------
def look_at(center, eye, up, W, H, vfov=60.0, z_near=0.01, z_far=1000.0):
    center, eye, up = (np64(v).reshape(3) for v in (center, eye, up))
    f = (center - eye) / np.sqrt(((center - eye) ** 2).sum())
    r = np.cross(f, up)
    r = r / np.sqrt((r ** 2).sum())
    d = np.cross(f, r)
    R = np.stack([r, d, f], axis=1)                     # camera to world, columns [r d f]
    w2c = np.concatenate([R.T, -(R.T @ eye)[:, None]], axis=1)
    fx = (H / 2) / np.tan(np.deg2rad(vfov) / 2)
    return Camera(w2c, fx, fx, W / 2, H / 2, W, H, z_near, z_far)


def follow_camera(c2w, W, H, vfov=60.0):
    c2w = np64(c2w)
    R = c2w[:3, :3]
    center = c2w[:3, 3]
    eye = center + np.array([0, -.6, -1.5]) @ R.T
    up = np.array([0, -1.0, 0]) @ R.T
    return look_at(center, eye, up, W, H, vfov)


def view_camera(scene, i, z_near=0.01, z_far=1000.0):
    H, W = (int(v) for v in scene.imgs[i].shape[:2])
    f = float(scene.focals[i])
    return Camera(np.linalg.inv(np64(scene.cams2world[i]))[:3], f, f, W / 2, H / 2, W, H, z_near, z_far)


def pose_camera(c2w, f, W, H, z_near=0.01, z_far=100.0):
    """a camera at the pose c2w with fx = fy = f and the principal point at the centre"""
    return Camera(np.linalg.inv(np64(c2w))[:3], float(f), float(f), W / 2, H / 2, W, H, z_near, z_far)
