"""Scene export: GLB / PLY point clouds and meshes from a ``SceneState`` (demo/gradio.py:75-156 ``get_3D_model_from_scene`` /
``_convert_scene_output_to_glb``), without trimesh.

Host planning (``scene_transform``, ``view_matrices``, ``camera_mask``, ``camera_frustums``), the device pass (``SceneExporter``: one
count + scan for up to 8 thresholds, one ordered scatter per threshold straight into file layout; csrc/export.hip through the C ABI)
and the two containers (``write_glb``, ``write_ply``).  The packed buffers leave the device through one pinned host buffer.

Differences from the reference, all in DESIGN.md: ``local_pointmaps=True`` applies ``S @ cams2world[i]`` (composed in fp64) to
``pts3d_local`` in one pass (the reference rounds to fp32 after ``geotrf``); a camera is a wireframe frustum (one LINES primitive), not
dust3r.viz's cone with a textured image, so ``transparent_cams`` has no effect; mesh colours are per vertex.
"""
import ctypes as C
import json
import os
import struct

import numpy as np
import torch

from . import _lib

# dust3r.viz settings data (written from memory of upstream; that module is not a dependency)
OPENGL = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], dtype=np.float64)
CAM_COLORS = [(255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 0, 255), (255, 204, 0), (0, 204, 204), (128, 255, 255), (255, 128, 255),
              (255, 255, 128), (0, 0, 0), (128, 128, 128)]
# get_reconstruction.py's threshold list
REFERENCE_THRESHOLDS = (6.0, 5.0, 4.0, 3.0, 2.5, 2.0, 1.5, 1.05)
MAX_THR = _lib.EXPORT_MAX_THR


# ------------------------------------------------------------------------------------------------------------------------------------
# host planning
# ------------------------------------------------------------------------------------------------------------------------------------
def rot_y(deg):
    """scipy's Rotation.from_euler('y', rad).as_matrix() as a 4x4: the quaternion (0, sin(a/2), 0, cos(a/2)) expanded the way scipy does,
    so that 180 degrees gives the same +-1.2e-16 off-diagonal terms."""
    a = np.deg2rad(deg)
    y, w = np.sin(a / 2), np.cos(a / 2)
    n = np.sqrt(y * y + w * w)
    y, w = y / n, w / n
    y2, w2, yw = y * y, w * w, y * w
    m = np.eye(4)
    m[0, 0] = -y2 + w2
    m[1, 1] = y2 + w2
    m[2, 2] = -y2 + w2
    m[0, 2] = 2 * yw
    m[2, 0] = -2 * yw
    return m


def _np64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def scene_transform(cam0):
    """S = inv(cams2world[0] @ OPENGL @ rot_y(180)) in fp64 (demo/gradio.py:114-116)."""
    return np.linalg.inv(_np64(cam0) @ OPENGL @ rot_y(180))


def view_matrices(cams2world, local_pointmaps=False):
    """-> (S [4,4], M [n,3,4]) fp64: M_i = S for pts3d, S @ cams2world[i] for pts3d_local."""
    S = scene_transform(cams2world[0])
    if local_pointmaps:
        M = np.stack([(S @ _np64(c))[:3] for c in cams2world])
    else:
        M = np.stack([S[:3] for _ in cams2world])
    return S, np.ascontiguousarray(M)


def camera_mask(x_out, camera_conf_thr):
    """demo/gradio.py:152: a view keeps its camera when its median confidence reaches the threshold."""
    return [bool(x["conf"].median() >= camera_conf_thr) for x in x_out]


def camera_frustums(scene, S, cam_size, mask):
    """-> (vertices float32 [5 m, 3], colours uint8 [5 m, 4], line indices uint32 [16 m]) of the m kept cameras: apex at the camera
    centre, four corners at depth ``cam_size`` through the image corners (focal, (W, H)), transformed by S in fp64."""
    verts, cols, idx = [], [], []
    edges = np.array([0, 1, 0, 2, 0, 3, 0, 4, 1, 2, 2, 3, 3, 4, 4, 1], dtype=np.uint32)
    for i, keep in enumerate(mask):
        if not keep:
            continue
        H, W = (int(v) for v in scene.imgs[i].shape[:2])
        f = float(scene.focals[i])
        x, y, d = 0.5 * W / f * cam_size, 0.5 * H / f * cam_size, float(cam_size)
        local = np.array([[0, 0, 0, 1], [-x, -y, d, 1], [x, -y, d, 1], [x, y, d, 1], [-x, y, d, 1]], dtype=np.float64)
        world = local @ (S @ _np64(scene.cams2world[i])).T
        idx.append(edges + np.uint32(5 * len(verts)))
        verts.append(world[:, :3].astype(np.float32))
        cols.append(np.tile(np.array(CAM_COLORS[i % len(CAM_COLORS)] + (255,), dtype=np.uint8), (5, 1)))
    if not verts:
        return None
    return np.concatenate(verts), np.concatenate(cols), np.concatenate(idx)


# ------------------------------------------------------------------------------------------------------------------------------------
# containers
# ------------------------------------------------------------------------------------------------------------------------------------
def _pad4(b, fill):
    return b + fill * (-len(b) % 4)


def write_glb(path, positions, colors, pos_min, pos_max, faces=None, cameras=None):
    """glTF 2.0 binary: one mesh; primitive 0 = the points (mode 0) or, with ``faces`` (uint32 [F, 3]), the triangles (mode 4, double-sided
    material); ``cameras`` = (vertices, colours, line indices) adds a LINES primitive.  positions float32 [N, 3], colours uint8 [N, 4]
    (COLOR_0 normalised UNSIGNED_BYTE VEC4).  Buffer views are 4-byte aligned; JSON padded with spaces, BIN with zeros."""
    positions = np.ascontiguousarray(positions, dtype="<f4").reshape(-1, 3)
    colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 4)
    assert len(positions) == len(colors) and len(positions) > 0
    chunks, views, accessors = [], [], []
    offset = 0

    def add(arr, ctype, atype, target, normalized=False, mn=None, mx=None):
        nonlocal offset
        raw = memoryview(arr).cast("B")
        views.append({"buffer": 0, "byteOffset": offset, "byteLength": len(raw), "target": target})
        acc = {"bufferView": len(views) - 1, "componentType": ctype, "count": len(arr), "type": atype}
        if normalized:
            acc["normalized"] = True
        if mn is not None:
            acc["min"], acc["max"] = [float(v) for v in mn], [float(v) for v in mx]
        accessors.append(acc)
        chunks.append(raw)
        pad = -len(raw) % 4
        if pad:
            chunks.append(b"\0" * pad)
        offset += len(raw) + pad
        return len(accessors) - 1

    prim = {"attributes": {"POSITION": add(positions, 5126, "VEC3", 34962, mn=pos_min, mx=pos_max),
                           "COLOR_0": add(colors, 5121, "VEC4", 34962, normalized=True)}, "mode": 0}
    doc = {"asset": {"version": "2.0", "generator": "must3r_amd"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}]}
    if faces is not None:
        faces = np.ascontiguousarray(faces, dtype="<u4").reshape(-1)
        prim["indices"] = add(faces, 5125, "SCALAR", 34963)
        prim["mode"] = 4
        prim["material"] = 0
        doc["materials"] = [{"doubleSided": True, "pbrMetallicRoughness": {"metallicFactor": 0.0, "roughnessFactor": 1.0}}]
    prims = [prim]
    if cameras is not None:
        cv, cc, ci = cameras
        cv = np.ascontiguousarray(cv, dtype="<f4").reshape(-1, 3)
        prims.append({"attributes": {"POSITION": add(cv, 5126, "VEC3", 34962, mn=cv.min(0), mx=cv.max(0)),
                                     "COLOR_0": add(np.ascontiguousarray(cc, dtype=np.uint8).reshape(-1, 4), 5121, "VEC4", 34962, normalized=True)},
                      "indices": add(np.ascontiguousarray(ci, dtype="<u4").reshape(-1), 5125, "SCALAR", 34963), "mode": 1})
    doc["meshes"] = [{"primitives": prims}]
    doc["bufferViews"], doc["accessors"], doc["buffers"] = views, accessors, [{"byteLength": offset}]
    js = _pad4(json.dumps(doc, separators=(",", ":")).encode("utf-8"), b" ")
    total = 12 + 8 + len(js) + 8 + offset
    if total >= 1 << 32:
        raise ValueError(f"write_glb: {total} bytes do not fit a GLB container (uint32 lengths)")
    tmp = path + ".part"
    with open(tmp, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, total))
        f.write(struct.pack("<I4s", len(js), b"JSON"))
        f.write(js)
        f.write(struct.pack("<I4s", offset, b"BIN\0"))
        for c in chunks:
            f.write(c)
    os.replace(tmp, path)
    return path


PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])


def write_ply(path, records):
    """binary_little_endian PLY of 16-byte vertex records x y z float32, red green blue alpha uchar (``PLY_DTYPE`` or raw bytes [N, 16])."""
    records = np.ascontiguousarray(records)
    raw = memoryview(records).cast("B")
    assert len(raw) % 16 == 0 and len(raw) > 0
    header = ("ply\nformat binary_little_endian 1.0\ncomment must3r_amd\n"
              f"element vertex {len(raw) // 16}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n")
    tmp = path + ".part"
    with open(tmp, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(raw)
    os.replace(tmp, path)
    return path


# ------------------------------------------------------------------------------------------------------------------------------------
# device pass
# ------------------------------------------------------------------------------------------------------------------------------------
def _as_device_f32(x, device):
    """fp32 contiguous on ``device``: device tensors are used in place, host tensors / arrays are uploaded."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if x.dtype != torch.float32:
        x = x.float()
    if not x.is_cuda:
        x = x.to(device, non_blocking=False)
    return x.contiguous()


class SceneExporter:
    """The views of a scene on the device + the C ABI calls.  ``count(thresholds, mesh)`` once, then ``points`` / ``faces`` per
    threshold index; ``vertices()`` in mesh mode.  Results are numpy views of one pinned host buffer, valid until the next call."""

    def __init__(self, views, matrices, device=None):
        """views: list of (conf [H, W], pts [H, W, 3], rgb [H, W, 3]) tensors or arrays, host or device; matrices: fp64 [n, 3, 4]."""
        self.lib = _lib.load()
        if device is None:
            device = next((t.device for v in views for t in v if isinstance(t, torch.Tensor) and t.is_cuda), None)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.tensors = []
        self.n = len(views)
        self.table = (_lib.ExportView * max(self.n, 1))()
        matrices = np.ascontiguousarray(matrices, dtype=np.float64).reshape(self.n, 12)
        self.n_pix = 0
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
            self.n_pix += H * W
        self.thr = None
        self.mesh = False
        self.scratch = None
        self.totals = None
        self._pinned = None
        self._dev = None
        self._minmax = torch.empty(6, dtype=torch.float32, device=self.device)

    def _stream(self):
        return C.c_void_p(_lib.stream_ptr(self.device))

    def _buffers(self, nbytes):
        nbytes = max(int(nbytes), 16)
        if self._dev is None or self._dev.numel() < nbytes:
            self._dev = None
            self._dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = None
            self._pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self._dev, self._pinned

    def _to_host(self, nbytes):
        self._pinned[:nbytes].copy_(self._dev[:nbytes], non_blocking=True)
        mm = self._minmax.cpu()            # synchronises the stream: the pinned buffer is complete
        return self._pinned[:nbytes].numpy(), mm.numpy()

    def count(self, thresholds, mesh=False):
        """-> totals per threshold (points; mesh: faces).  One read of every view's confidences, one scan, one small copy back."""
        thresholds = [float(t) for t in thresholds]
        K = len(thresholds)
        with torch.cuda.device(self.device):
            self.thr = (C.c_float * max(K, 1))(*thresholds)
            self.mesh = bool(mesh)
            nbytes = self.lib.must3r_hip_export_scratch_bytes(self.table, self.n, K, int(self.mesh))
            if nbytes == 0:
                _lib.check(1)
            if self.scratch is None or self.scratch.numel() < nbytes:
                self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            totals = (C.c_int64 * K)()
            _lib.check(self.lib.must3r_hip_export_count(self.table, self.n, self.thr, K, int(self.mesh), C.c_void_p(self.scratch.data_ptr()),
                                                        self.scratch.numel(), totals, self._stream()))
        self.totals = [int(t) for t in totals]
        return self.totals

    def points_device(self, k, layout=_lib.EXPORT_GLB):
        """scatter threshold k into the device buffer -> (uint8 device tensor of the packed bytes, n, minmax device tensor)"""
        n = self.totals[k]
        dev, _ = self._buffers(16 * n)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.must3r_hip_export_scatter_points(self.table, self.n, self.thr, len(self.totals), k, layout,
                                                                 C.c_void_p(self.scratch.data_ptr()), C.c_void_p(dev.data_ptr()),
                                                                 C.c_void_p(dev.data_ptr() + 12 * n), C.c_void_p(self._minmax.data_ptr()),
                                                                 self._stream()))
        return dev[:16 * n], n, self._minmax

    def points(self, k, layout=_lib.EXPORT_GLB):
        """GLB: (positions float32 [n, 3], colours uint8 [n, 4], min [3], max [3]); PLY: (records PLY_DTYPE [n], min, max)"""
        assert not self.mesh, "count() ran in mesh mode"
        _, n, _ = self.points_device(k, layout)
        host, mm = self._to_host(16 * n)
        if layout == _lib.EXPORT_PLY:
            return host.view(PLY_DTYPE), mm[:3], mm[3:]
        return host[:12 * n].view("<f4").reshape(n, 3), host[12 * n:].reshape(n, 4), mm[:3], mm[3:]

    def vertices(self):
        """mesh mode: every pixel of every view -> (positions float32 [N, 3], colours uint8 [N, 4], min, max); fresh arrays"""
        assert self.mesh, "count() ran in point mode"
        n = self.n_pix
        dev, _ = self._buffers(16 * n)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.must3r_hip_export_vertices(self.table, self.n, len(self.totals), C.c_void_p(self.scratch.data_ptr()),
                                                           C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr() + 12 * n),
                                                           C.c_void_p(self._minmax.data_ptr()), self._stream()))
        host, mm = self._to_host(16 * n)
        return host[:12 * n].view("<f4").reshape(n, 3).copy(), host[12 * n:].reshape(n, 4).copy(), mm[:3].copy(), mm[3:].copy()

    def faces_device(self, k):
        n = self.totals[k]
        dev, _ = self._buffers(12 * n)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.must3r_hip_export_scatter_faces(self.table, self.n, self.thr, len(self.totals), k,
                                                                C.c_void_p(self.scratch.data_ptr()), C.c_void_p(dev.data_ptr()), self._stream()))
        return dev[:12 * n], n

    def faces(self, k):
        """mesh mode: uint32 [n_faces, 3] of threshold k"""
        assert self.mesh, "count() ran in point mode"
        _, n = self.faces_device(k)
        host, _ = self._to_host(12 * n)
        return host.view("<u4").reshape(n, 3)


# ------------------------------------------------------------------------------------------------------------------------------------
# scene -> files
# ------------------------------------------------------------------------------------------------------------------------------------
def scene_views(scene, local_pointmaps=False):
    """-> list of (conf, pts, rgb) of a SceneState, as get_3D_model_from_scene picks them (demo/gradio.py:142-151)."""
    key = "pts3d_local" if local_pointmaps else "pts3d"
    return [(scene.x_out[i]["conf"], scene.x_out[i][key], scene.imgs[i]) for i in range(len(scene.imgs))]


def export_scene(outdir, scene, thresholds, filenames, as_pointcloud=True, transparent_cams=False, local_pointmaps=False, cam_size=0.05,
                 camera_conf_thr=0.0, verbose=False):
    """One file per threshold -> list of paths, None where a threshold selects nothing (no file is written for it).  All thresholds
    share one count + scan per chunk of 8; one scatter each.  ``transparent_cams`` is accepted and has no effect (wireframe cameras)."""
    thresholds = [float(t) for t in thresholds]
    assert len(thresholds) == len(filenames)
    ply = [str(f).endswith("ply") for f in filenames]
    if any(ply) and not as_pointcloud:
        raise ValueError("a .ply export is a point cloud: as_pointcloud=False (mesh) needs a .glb file name")
    S, M = view_matrices(scene.cams2world, local_pointmaps)
    exporter = SceneExporter(scene_views(scene, local_pointmaps), M)
    cameras = None
    if not all(ply):
        cameras = camera_frustums(scene, S, cam_size, camera_mask(scene.x_out, camera_conf_thr))
    os.makedirs(outdir, exist_ok=True)
    out = []
    verts = None
    for c0 in range(0, len(thresholds), MAX_THR):
        chunk = thresholds[c0:c0 + MAX_THR]
        totals = exporter.count(chunk, mesh=not as_pointcloud)
        for k, total in enumerate(totals):
            path = os.path.join(outdir, filenames[c0 + k])
            if total == 0:
                out.append(None)
                continue
            if verbose:
                print("(exporting 3D scene to", path, ")")
            if not as_pointcloud:
                if verts is None:
                    verts = exporter.vertices()
                write_glb(path, verts[0], verts[1], verts[2], verts[3], faces=exporter.faces(k), cameras=cameras)
            elif ply[c0 + k]:
                write_ply(path, exporter.points(k, _lib.EXPORT_PLY)[0])
            else:
                pos, col, mn, mx = exporter.points(k, _lib.EXPORT_GLB)
                write_glb(path, pos, col, mn, mx, cameras=cameras)
            out.append(path)
    return out
