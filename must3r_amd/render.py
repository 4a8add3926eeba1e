"""Headless scene rendering: a point rasteriser and a triangle rasteriser for previews of a ``SceneState`` or of a SLAM run's map (what the reference shows through
demo/viser.py and the open3d ``PipelineView`` of slam/slam.py), written as PNG frames.

Host planning in fp64 numpy (``view_camera``, ``look_at``, ``follow_camera``, ``orbit_cameras``), the device pass (``SceneRenderer``: one
splat launch over all cameras and all source pixels, one resolve; csrc/render.hip through the C ABI, and with ``mesh=True`` csrc/render_mesh.hip:
the two triangles per pixel quad that the export writes, into the same three images), ``colorize_grayscale`` for the grey panels and
``render_scene`` for the files.  The frames leave the device through one pinned host buffer.

The arithmetic order, the key layout and the tie rule are in DESIGN.md section 14 (triangles: 14.1).  Not built: near-plane clipping and culling
of stretched triangles, textures, anti-aliasing, hole filling, a mesh of the SLAM map, a live per-frame SLAM view and any interactive server.
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .export import SceneExporter, _as_device_f32, _np64, scene_views

Camera = collections.namedtuple("Camera", "w2c fx fy cx cy W H z_near z_far")
Camera.__doc__ = """One pinhole camera: ``w2c`` fp64 [3, 4] world to camera in OpenCV axes (x right, y down, z forward), intrinsics in pixels,
the image size and the depth range (0 < z_near <= z_far)."""
Z_NEAR, Z_FAR = 0.01, 1000.0
SCRATCH_BUDGET = 256 << 20      # bytes of z-buffer scratch one native call may use: 32 M target pixels


# ------------------------------------------------------------------------------------------------------------------------------------
# camera planning (host, fp64)
# ------------------------------------------------------------------------------------------------------------------------------------
def _rigid_inverse(c2w):
    c2w = _np64(c2w)
    R, t = c2w[:3, :3], c2w[:3, 3]
    return np.concatenate([R.T, -(R.T @ t)[:, None]], axis=1)


def _focal_of_vfov(H, vfov):
    return (H / 2) / np.tan(np.deg2rad(vfov) / 2)


def view_camera(scene, i, z_near=Z_NEAR, z_far=Z_FAR):
    """The camera of view i as the scene estimates it: the inverse of ``cams2world[i]``, fx = fy = ``focals[i]``, the principal point at the
    centre and the size of image i -- the rendered cloud can be laid next to the input photo."""
    H, W = (int(v) for v in scene.imgs[i].shape[:2])
    f = float(scene.focals[i])
    return Camera(np.linalg.inv(_np64(scene.cams2world[i]))[:3], f, f, W / 2, H / 2, W, H, z_near, z_far)


def look_at(center, eye, up, W, H, vfov=60.0, z_near=Z_NEAR, z_far=Z_FAR):
    """A camera at ``eye`` looking at ``center``: forward f = normalised (center - eye), right r = normalised (f x up), down d = f x r, the
    camera-to-world rotation has the columns [r d f]; fy = fx = (H / 2) / tan(vfov / 2), the principal point at the centre."""
    center, eye, up = (_np64(v).reshape(3) for v in (center, eye, up))
    f = center - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, eye
    fx = _focal_of_vfov(H, vfov)
    return Camera(_rigid_inverse(c2w), fx, fx, W / 2, H / 2, int(W), int(H), z_near, z_far)


def follow_camera(c2w, W, H, vfov=60.0, z_near=Z_NEAR, z_far=Z_FAR):
    """The reference's ``reset_view`` (slam/slam.py:476-486): look at the camera centre of ``c2w`` from behind and slightly above it,
    eye = center + [0, -.6, -1.5] @ R.T, up = [0, -1, 0] @ R.T."""
    c2w = _np64(c2w)
    Rt = c2w[:3, :3].T
    center = c2w[:3, 3]
    eye = center + np.array([0, -.6, -1.5]) @ Rt
    up = np.array([0, -1.0, 0]) @ Rt
    return look_at(center, eye, up, W, H, vfov, z_near, z_far)


def _kept_box(views, matrices, thr):
    """min / max of the points kept at ``thr``: the exporter's one small read"""
    ex = SceneExporter(views, matrices)
    if ex.count([thr])[0] == 0:
        raise ValueError(f"orbit_cameras: no point has confidence >= {thr}")
    _, _, mm = ex.points_device(0)
    mm = mm.cpu().numpy().astype(np.float64)
    return mm[:3], mm[3:]


def orbit_box(mn, mx, c2w0, n, W, H, vfov=60.0, elevation_deg=20.0):
    """``orbit_cameras`` from the box itself: n cameras on a circle about the centre of the box [mn, mx], the axis the up direction of the
    pose ``c2w0``, at the distance where the box's bounding sphere fits the narrower of the two fields of view; the depth range encloses the
    sphere."""
    mn, mx, c2w0 = _np64(mn), _np64(mx), _np64(c2w0)
    centre = 0.5 * (mn + mx)
    rs = max(0.5 * float(np.linalg.norm(mx - mn)), 1e-6)
    fx = _focal_of_vfov(H, vfov)
    half = min(np.deg2rad(vfov) / 2, np.arctan((W / 2) / fx))
    dist = rs / np.sin(half)
    axis = -c2w0[:3, 1]                       # [0, -1, 0] @ R.T
    e1 = -c2w0[:3, 2]                         # the first camera stands behind view 0
    e2 = np.cross(axis, e1)
    el = np.deg2rad(elevation_deg)
    cams = []
    for k in range(n):
        a = 2 * np.pi * k / n
        eye = centre + dist * (np.cos(el) * (np.cos(a) * e1 + np.sin(a) * e2) + np.sin(el) * axis)
        cams.append(look_at(centre, eye, axis, W, H, vfov, z_near=0.5 * (dist - rs), z_far=2.0 * (dist + rs)))
    return cams


def orbit_cameras(scene, n, thr, W, H, vfov=60.0, elevation_deg=20.0, local_pointmaps=False):
    """n cameras on a circle about the centre of the bounding box of the points kept at ``thr`` (``orbit_box``)."""
    mn, mx = _kept_box(scene_views(scene, local_pointmaps), _matrices(scene, local_pointmaps), thr)
    return orbit_box(mn, mx, scene.cams2world[0], n, W, H, vfov, elevation_deg)


def _matrices(scene, local_pointmaps):
    """identity for ``pts3d``; ``cams2world[i]`` for ``pts3d_local``: the points stay in the frame of ``cams2world``"""
    n = len(scene.imgs)
    if not local_pointmaps:
        return np.tile(np.eye(4)[:3], (n, 1, 1))
    return np.stack([_np64(c)[:3] for c in scene.cams2world])


# ------------------------------------------------------------------------------------------------------------------------------------
# device pass
# ------------------------------------------------------------------------------------------------------------------------------------
def colorize_grayscale(x):
    """demo/viser.py:22-25 on the device: (x - min) / (max - min + 1e-9) replicated to three channels"""
    mind, maxd = x.min(), x.max()
    x = (x - mind) / (maxd - mind + 1e-9)
    return torch.stack([x, x, x], dim=-1)


class SceneRenderer:
    """The views of a scene on the device + the C ABI call.  ``views`` as ``SceneExporter`` takes them; ``matrices`` fp64 [n, 3, 4], None =
    the identity (the points stay in the frame they are in)."""

    def __init__(self, views, matrices=None, device=None, scratch_budget=SCRATCH_BUDGET):
        self.lib = _lib.load()
        if device is None:
            device = next((t.device for v in views for t in v if isinstance(t, torch.Tensor) and t.is_cuda), None)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n = len(views)
        if matrices is None:
            matrices = np.tile(np.eye(4)[:3], (self.n, 1, 1))
        matrices = np.ascontiguousarray(matrices, dtype=np.float64).reshape(self.n, 12)
        self.tensors = []
        self.table = (_lib.ExportView * max(self.n, 1))()
        for i, (conf, pts, rgb) in enumerate(views):
            conf, pts, rgb = (_as_device_f32(t, self.device) for t in (conf, pts, rgb))
            H, W = conf.shape
            if tuple(pts.shape) != (H, W, 3) or tuple(rgb.shape) != (H, W, 3):
                raise ValueError(f"view {i}: conf {tuple(conf.shape)}, pts {tuple(pts.shape)} and rgb {tuple(rgb.shape)} do not match")
            self.tensors.append((conf, pts, rgb))
            e = self.table[i]
            e.conf, e.pts, e.rgb, e.H, e.W = conf.data_ptr(), pts.data_ptr(), rgb.data_ptr(), H, W
            for j in range(12):
                e.M[j] = matrices[i, j]
        self.scratch_budget = int(scratch_budget)
        self.scratch = None

    def _call(self, cams, thr, point_size, background, out, mesh=False):
        """one native call: cameras of one size -> the slices ``out`` = dict(rgb, depth, index) of device tensors (or None)"""
        table = (_lib.RenderCamera * len(cams))()
        for e, c in zip(table, cams):
            w2c = np.ascontiguousarray(c.w2c, dtype=np.float64).reshape(12)
            for j in range(12):
                e.w2c[j] = w2c[j]
            e.fx, e.fy, e.cx, e.cy, e.z_near, e.z_far, e.W, e.H = c.fx, c.fy, c.cx, c.cy, c.z_near, c.z_far, c.W, c.H
        d = _lib.RenderMeshDesc() if mesh else _lib.RenderDesc()
        d.views, d.cams, d.n_views, d.n_cams = self.table, table, self.n, len(cams)
        d.thr = float(thr)
        if not mesh:
            d.point_size = int(point_size)
        for a in range(3):
            d.background[a] = int(background[a])
        scratch_bytes, run = ((self.lib.must3r_hip_render_mesh_scratch_bytes, self.lib.must3r_hip_render_mesh) if mesh else
                              (self.lib.must3r_hip_render_scratch_bytes, self.lib.must3r_hip_render))
        nbytes = scratch_bytes(C.byref(d))
        if nbytes == 0:
            _lib.check(1)
        if self.scratch is None or self.scratch.numel() < nbytes:
            self.scratch = None
            self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        d.scratch, d.scratch_bytes = self.scratch.data_ptr(), self.scratch.numel()
        d.rgb, d.depth, d.index = (None if out[k] is None else out[k].data_ptr() for k in ("rgb", "depth", "index"))
        d.stream = _lib.stream_ptr(self.device)
        _lib.check(run(C.byref(d)))

    def render(self, cameras, thr, point_size=1, background=(255, 255, 255), want=("rgb", "depth", "index"), mesh=False):
        """-> one dict per camera, in the cameras' order, of device tensors: ``rgb`` uint8 [H, W, 3], ``depth`` float32 [H, W] (+inf where
        nothing landed), ``index`` uint32 [H, W] (0xFFFFFFFF there; else views in order, pixels row-major) -- those named in ``want``.
        Cameras are grouped by (W, H), each group is one tensor per output, and a group goes to the library in chunks whose z-buffers stay
        inside the scratch budget.  Everything is enqueued on the current stream; nothing is read back.
        ``mesh=True`` draws the triangles of the exported mesh instead (two per quad of every view's pixel grid, perspective-correct depth and
        colour): ``index`` is then the triangle id, 2 x (source index of the quad's first pixel) + (0 upper-left, 1 lower-right triangle), and
        ``point_size`` must be left at 1."""
        cameras = list(cameras)
        unknown = set(want) - {"rgb", "depth", "index"}
        if unknown or not want:
            raise ValueError(f"render: want {tuple(want)} is not a non-empty subset of ('rgb', 'depth', 'index')")
        if mesh and int(point_size) != 1:
            raise ValueError(f"render: point_size {point_size} with mesh=True; triangles have no point size, leave it at 1")
        if not 1 <= int(point_size) <= _lib.RENDER_MAX_POINT_SIZE:
            raise ValueError(f"render: point_size {point_size} is outside [1, {_lib.RENDER_MAX_POINT_SIZE}]")
        result = [None] * len(cameras)
        groups = {}
        for i, c in enumerate(cameras):
            groups.setdefault((int(c.W), int(c.H)), []).append(i)
        spec = {"rgb": ((3,), torch.uint8), "depth": ((), torch.float32), "index": ((), torch.uint32)}
        with torch.cuda.device(self.device):
            for (W, H), ids in groups.items():
                if W <= 0 or H <= 0:
                    raise ValueError(f"render: camera image size {W} x {H}")
                full = {k: torch.empty((len(ids), H, W) + spec[k][0], dtype=spec[k][1], device=self.device) if k in want else None for k in spec}
                chunk = max(1, self.scratch_budget // (8 * W * H))
                for c0 in range(0, len(ids), chunk):
                    sel = ids[c0:c0 + chunk]
                    self._call([cameras[i] for i in sel], thr, point_size, background,
                               {k: None if t is None else t[c0:c0 + len(sel)] for k, t in full.items()}, mesh)
                for j, i in enumerate(ids):
                    result[i] = {k: t[j] for k, t in full.items() if t is not None}
        return result


# ------------------------------------------------------------------------------------------------------------------------------------
# scene -> PNG frames
# ------------------------------------------------------------------------------------------------------------------------------------
class _FrameWriter:
    """device images -> PNG files through ONE pinned host buffer (as the export's)"""

    def __init__(self):
        self._pinned = None

    def write(self, path, img):
        """img: uint8 device tensor [H, W, 3]"""
        import PIL.Image
        img = img.contiguous()
        n = img.numel()
        if self._pinned is None or self._pinned.numel() < n:
            self._pinned = None
            self._pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        host = self._pinned[:n].view(img.shape)
        host.copy_(img, non_blocking=True)
        torch.cuda.current_stream(img.device).synchronize()
        PIL.Image.fromarray(host.numpy()).save(path)
        return path


def depth_panel(depth):
    """the grey panel of a rendered depth image: ``colorize_grayscale`` over the pixels something landed on, empty pixels black -> uint8 [H, W, 3]"""
    hit = torch.isfinite(depth)
    if not bool(hit.any()):
        return torch.zeros(depth.shape + (3,), dtype=torch.uint8, device=depth.device)
    lo = depth[hit].min()
    grey = colorize_grayscale(torch.where(hit, depth, lo))
    return (torch.where(hit[..., None], grey, torch.zeros_like(grey)) * 255).round().to(torch.uint8)


def render_views(outdir, views, matrices, cameras, thr=3.0, point_size=2, depth=False, background=(255, 255, 255), start=0, batch=32, mesh=False):
    """``render_scene`` for any list of (conf, pts, rgb) views: ``frame_%05d.png`` (and ``depth_%05d.png``) from ``start`` on, ``batch``
    cameras per render call -> the list of frame paths.  ``mesh=True``: triangles, and ``point_size`` is not used."""
    os.makedirs(outdir, exist_ok=True)
    renderer = SceneRenderer(views, matrices)
    writer = _FrameWriter()
    cameras = list(cameras)
    paths = []
    for c0 in range(0, len(cameras), batch):
        images = renderer.render(cameras[c0:c0 + batch], thr, 1 if mesh else point_size, background, want=("rgb", "depth") if depth else ("rgb",),
                                 mesh=mesh)
        for j, im in enumerate(images):
            k = start + c0 + j
            paths.append(writer.write(os.path.join(outdir, "frame_%05d.png" % k), im["rgb"]))
            if depth:
                writer.write(os.path.join(outdir, "depth_%05d.png" % k), depth_panel(im["depth"]))
    return paths


def render_scene(outdir, scene, cameras, thr=3.0, point_size=2, local_pointmaps=False, depth=False, background=(255, 255, 255), start=0, mesh=False):
    """One ``frame_%05d.png`` per camera of the points of ``scene`` with confidence >= ``thr``; ``depth=True`` also writes
    ``depth_%05d.png``, the grey panel of the rendered depth with empty pixels black -> the list of frame paths.  ``mesh=True`` draws the
    scene's mesh (what ``get_3D_model_from_scene(as_pointcloud=False)`` exports) instead of its points."""
    return render_views(outdir, scene_views(scene, local_pointmaps), _matrices(scene, local_pointmaps), cameras, thr, point_size, depth,
                        background, start, mesh=mesh)
