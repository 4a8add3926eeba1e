"""numpy restatement of the scene export (what must3r_amd.export must produce) and an independent reader of GLB / PLY files.

Written from the description of the method, not from any exporter's code:
  selection   conf >= thr (NaN never passes), views in order, row-major inside a view
  position    per output row of the view's 3x4 fp64 matrix: ((m0 x + m1 y) + m2 z) + m3, every operation an fp64 numpy ufunc (numpy does
              not fuse), then one rounding to fp32
  colour      rint(clip(c, 0, 1) * 255) in fp32 -> uint8, alpha 255
  mesh        vertices = all pixels; per view the triangles (a,b,c'), (c',b,a), (b,c',d), (d,c',b) of every quad, a triangle kept when
              its three corners pass, group after group in quad row-major order, indices offset by the pixels of the views before
The reader parses the containers byte by byte (struct / json) and shares nothing with must3r_amd.export's writers.
"""
import json
import struct

import numpy as np

OPENGL = np.diag([1.0, -1.0, -1.0, 1.0])
THRESHOLDS = (6.0, 5.0, 4.0, 3.0, 2.5, 2.0, 1.5, 1.05)


def np32(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float32)


def np64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def scene_transform(cam0):
    a = np.deg2rad(180.0)
    rot = np.eye(4)
    rot[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    return np.linalg.inv(np64(cam0) @ OPENGL @ rot)


def view_matrices(cams2world, local_pointmaps):
    S = scene_transform(cams2world[0])
    return [(S @ np64(c))[:3] if local_pointmaps else S[:3] for c in cams2world]


def transform(M, pts):
    """M fp64 [3, 4], pts fp32 [..., 3] -> fp32 [..., 3]: fp64 arithmetic in the stated order, one rounding"""
    p = np32(pts).astype(np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    M = np64(M)
    rows = [((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3] for a in range(3)]
    return np.stack(rows, axis=-1).astype(np.float32)


def quantise(rgb):
    c = np.clip(np32(rgb), np.float32(0), np.float32(1)) * np.float32(255)
    assert c.dtype == np.float32
    out = np.full(c.shape[:-1] + (4,), 255, dtype=np.uint8)
    out[..., :3] = np.rint(c).astype(np.uint8)
    return out


def select(conf, thr):
    """fp32 comparison, the threshold rounded to fp32 first: what torch does for ``conf_fp32_tensor >= python_float``"""
    return np32(conf) >= np.float32(thr)


def pointcloud(views, matrices, thr):
    """views: list of (conf [H, W], pts [H, W, 3], rgb [H, W, 3]) -> positions fp32 [n, 3], colours uint8 [n, 4]"""
    pos, col = [], []
    for (conf, pts, rgb), M in zip(views, matrices):
        m = select(conf, thr)
        pos.append(transform(M, np32(pts)[m]))
        col.append(quantise(np32(rgb)[m]))
    return np.concatenate(pos).reshape(-1, 3), np.concatenate(col).reshape(-1, 4)


def ply_records(pos, col):
    rec = np.zeros(len(pos), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
    rec["x"], rec["y"], rec["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    rec["red"], rec["green"], rec["blue"], rec["alpha"] = col[:, 0], col[:, 1], col[:, 2], col[:, 3]
    return rec


def view_faces(valid):
    """bool [H, W] -> int64 [f, 3]: the surviving triangles of one view, local vertex indices"""
    H, W = valid.shape
    idx = np.arange(H * W).reshape(H, W)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.concatenate([np.stack(t, axis=1) for t in ((a, b, c), (c, b, a), (b, c, d), (d, c, b))])
    keep = valid.ravel()[faces].all(axis=-1)
    return faces[keep]


def mesh(views, matrices, thr):
    """-> vertices fp32 [N, 3], colours uint8 [N, 4], faces uint32 [F, 3]"""
    pos, col, faces, base = [], [], [], 0
    for (conf, pts, rgb), M in zip(views, matrices):
        pos.append(transform(M, np32(pts).reshape(-1, 3)))
        col.append(quantise(np32(rgb).reshape(-1, 3)))
        faces.append(view_faces(select(conf, thr)) + base)
        base += np32(conf).size
    return np.concatenate(pos), np.concatenate(col), np.concatenate(faces).astype(np.uint32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------------------------
# independent reader
# ------------------------------------------------------------------------------------------------------------------------------------
_COMPONENT = {5120: "i1", 5121: "u1", 5122: "<i2", 5123: "<u2", 5125: "<u4", 5126: "<f4"}
_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}


def read_glb(path):
    """-> dict(json=..., length=..., chunks=[(type, length)], primitives=[dict(mode, material, POSITION, COLOR_0, indices, accessors)])
    Asserts the container rules: magic, version 2, total length = file size, chunk lengths multiples of 4, JSON then BIN, JSON padded with
    spaces, buffer views inside the buffer and 4-byte aligned."""
    raw = open(path, "rb").read()
    magic, version, length = struct.unpack_from("<4sII", raw, 0)
    assert magic == b"glTF" and version == 2
    assert length == len(raw), (length, len(raw))
    off, chunks = 12, []
    while off < len(raw):
        clen, ctype = struct.unpack_from("<I4s", raw, off)
        assert clen % 4 == 0 and (off + 8) % 4 == 0
        chunks.append((ctype, raw[off + 8: off + 8 + clen]))
        off += 8 + clen
    assert off == len(raw)
    assert [c[0] for c in chunks] == [b"JSON", b"BIN\0"]
    js = chunks[0][1]
    assert js.rstrip(b" ") == js.strip() and not js.rstrip(b" ").endswith(b"\0")
    doc = json.loads(js.decode("utf-8"))
    binary = chunks[1][1]
    assert doc["asset"]["version"] == "2.0"
    assert len(doc["buffers"]) == 1 and doc["buffers"][0]["byteLength"] <= len(binary) < doc["buffers"][0]["byteLength"] + 4
    assert not any(binary[doc["buffers"][0]["byteLength"]:])

    def accessor(i):
        acc = doc["accessors"][i]
        bv = doc["bufferViews"][acc["bufferView"]]
        assert bv["byteOffset"] % 4 == 0 and bv["byteOffset"] + bv["byteLength"] <= doc["buffers"][0]["byteLength"]
        dt, w = np.dtype(_COMPONENT[acc["componentType"]]), _WIDTH[acc["type"]]
        n = acc["count"] * w
        start = bv["byteOffset"] + acc.get("byteOffset", 0)
        assert n * dt.itemsize <= bv["byteLength"]
        arr = np.frombuffer(binary, dtype=dt, count=n, offset=start)
        return arr.reshape(acc["count"], w) if w > 1 else arr

    prims = []
    scene = doc["scenes"][doc["scene"]]
    for node in scene["nodes"]:
        for p in doc["meshes"][doc["nodes"][node]["mesh"]]["primitives"]:
            out = dict(mode=p.get("mode", 4), material=None if "material" not in p else doc["materials"][p["material"]],
                       accessors={k: doc["accessors"][v] for k, v in p["attributes"].items()})
            for k, v in p["attributes"].items():
                out[k] = accessor(v)
            out["indices"] = accessor(p["indices"]) if "indices" in p else None
            prims.append(out)
    return dict(json=doc, length=length, chunks=[(c[0], len(c[1])) for c in chunks], primitives=prims)


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "uchar": "u1", "uint8": "u1", "double": "<f8", "int": "<i4", "uint": "<u4"}


def read_ply(path):
    """-> structured array of the vertex element of a binary_little_endian PLY"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    count, fields, in_vertex = None, [], False
    for ln in lines[2:]:
        tok = ln.split()
        if not tok or tok[0] == "comment":
            continue
        if tok[0] == "element":
            in_vertex = tok[1] == "vertex"
            if in_vertex:
                count = int(tok[2])
        elif tok[0] == "property" and in_vertex:
            fields.append((tok[2], _PLY_TYPES[tok[1]]))
    dt = np.dtype(fields)
    assert len(raw) - end == count * dt.itemsize, (len(raw) - end, count, dt.itemsize)
    return np.frombuffer(raw, dtype=dt, count=count, offset=end)


# ------------------------------------------------------------------------------------------------------------------------------------
# seeded fake scenes (the fields of must3r_amd.demo.SceneState that the export reads)
# ------------------------------------------------------------------------------------------------------------------------------------
class FakeScene:
    def __init__(self, x_out, imgs, focals, cams2world):
        self.x_out, self.imgs, self.focals, self.cams2world = x_out, imgs, focals, cams2world
        self.true_shape = [tuple(x["conf"].shape) for x in x_out]
        self.image_list = [f"view{i}.png" for i in range(len(x_out))]


def make_scene(shapes, seed=0, device=None):
    """views of the given (H, W): pts3d_local in front of the camera, a rigid pose per view (view 0 is NOT the identity), pts3d = the
    fp32 geotrf of the local points, conf = 1 + exp(randn), colours a little outside [0, 1] so that the clip matters.
    device=None: host scene as must3r_inference returns it (torch host tensors, numpy images); else everything on that device."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x_out, imgs, focals, cams = [], [], [], []
    for i, (H, W) in enumerate(shapes):
        local = torch.randn((H, W, 3), generator=g) * 0.3
        local[..., 2] = local[..., 2].abs() + 1.0 + 0.1 * i
        q, _ = torch.linalg.qr(torch.randn((3, 3), generator=g, dtype=torch.float64))
        if torch.det(q) < 0:
            q[:, 0] = -q[:, 0]
        c2w = torch.eye(4)
        c2w[:3, :3] = q.float()
        c2w[:3, 3] = torch.randn(3, generator=g) * 0.5
        pts = local @ c2w[:3, :3].T + c2w[:3, 3]
        conf = 1.0 + torch.exp(torch.randn((H, W), generator=g))
        rgb = torch.rand((H, W, 3), generator=g) * 1.2 - 0.1
        x = dict(pts3d=pts, pts3d_local=local, conf=conf, focal=torch.tensor(10.0 + i), c2w=c2w)
        if device is not None:
            x = {k: v.to(device) for k, v in x.items()}
            rgb = rgb.to(device)
        else:
            rgb = rgb.numpy()
        x_out.append(x)
        imgs.append(rgb)
        focals.append(10.0 + i)
        cams.append(c2w)
    return FakeScene(x_out, imgs, focals, cams)


def scene_views(scene, local_pointmaps=False):
    key = "pts3d_local" if local_pointmaps else "pts3d"
    return [(np32(x["conf"]), np32(x[key]), np32(im)) for x, im in zip(scene.x_out, scene.imgs)]
