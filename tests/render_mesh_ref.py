"""numpy restatement of the triangle rasteriser (what must3r_amd.render with ``mesh=True`` / csrc/render_mesh.hip must produce), written from the
description of the rule in include/must3r_hip.h ("scene rendering, triangles"), not from the kernels or from csrc/render_tri.hpp:

  triangles   export_ref.view_faces of the confidence mask gives the kept set; kind 0 of the quad anchored at i is (i, i + 1, i + W), kind 1 is
              (i + 1, i + W, i + W + 1); id = 2 (global source index of the anchor) + kind
  vertices    render_ref.compose / render_ref.project per view and camera; a triangle is dropped when a corner has a non-finite x, y, z, u, v or
              a Z outside [z_near, z_far]
  candidates  columns ceil(min u - 0.5) .. floor(max u - 0.5), rows likewise, clipped in fp64
  coverage    E_jk(p) = (u_k - u_j) (py - v_j) - (v_k - v_j) (px - u_j); s0 = E_01, s1 = E_12, s2 = -E_02; den = (s0 + s1) + s2 finite and not
              zero, all s >= 0 or all s <= 0
  depth       lam = (s1, s2, s0) / den; t_k = lam_k (1.0 / Z_k); Zp = 1.0 / ((t0 + t1) + t2); key (bits(fp32 Zp) << 32) | id under np.minimum.at
  resolve     colour ((t0 c0 + t1 c1) + t2 c2) Zp per channel in fp64, one rounding to fp32, export_ref.quantise
Every operation is an fp64 numpy ufunc of its own (numpy does not fuse).  A triangle is one Python iteration and its candidate box one array.

Three planted defects, each behind a flag of ``contenders`` / ``render``: ``exclusive`` (edges with s == 0 are outside), ``affine`` (depth
and colour weights lam_k instead of lam_k / Z_k) and ``e20`` (the third edge evaluated from corner 2, E_20, instead of -E_02: the same number in
exact arithmetic, other bits).
"""
import numpy as np

from export_ref import np32, quantise, select, view_faces
from render_ref import EMPTY, compose, project

DROPS = ("conf", "nonfinite", "near", "far", "off_image", "no_sample")


def view_triangles(conf, thr):
    """-> list of (local anchor, kind, (i0, i1, i2)) of the view's kept triangles, anchors ascending, kind 0 before kind 1; and the number of
    triangles the confidence test removed"""
    conf = np32(conf)
    H, W = conf.shape
    kept = {tuple(int(x) for x in f) for f in view_faces(select(conf, thr))}
    out, dropped = [], 0
    for r in range(H - 1):
        for c in range(W - 1):
            i = r * W + c
            for kind, corners in ((0, (i, i + 1, i + W)), (1, (i + 1, i + W, i + W + 1))):
                if corners in kept:
                    assert tuple(reversed(corners)) in kept          # the export's second winding: drawn once
                    out.append((i, kind, corners))
                else:
                    dropped += 1
    return out, dropped


def _edge(uj, vj, uk, vk, px, py):
    return (uk - uj) * (py - vj) - (vk - vj) * (px - uj)


def _span(mn, mx, n):
    """sample indices k in [0, n) with mn <= k + 0.5 <= mx, fp64 until the range is known -> (lo, hi, clipped), or "off_image" when the unclipped
    range lies outside [0, n), or "no_sample" when it is empty"""
    a, b = np.ceil(mn - 0.5), np.floor(mx - 0.5)
    if not a <= b:
        return "no_sample"
    if a > n - 1 or b < 0:
        return "off_image"
    lo, hi = max(a, 0.0), min(b, float(n - 1))
    return int(lo), int(hi), bool(lo != a or hi != b)


def contenders(views, matrices, cam, thr, exclusive=False, affine=False, e20=False):
    """-> dict(pix int64 [m], key uint64 [m], t fp64 [m, 3], Zp fp64 [m], Zc fp64 [m] (the factor of the colour sum: Zp), corners int64 [m, 3] global source indices, stats, boxes):
    every (covered target pixel, key) pair of one camera before the minimum.  stats: triangles in all, dropped for each reason of DROPS (the
    first that applies, in that order; off_image = the bounding box misses the image, no_sample = it holds no pixel centre), drawn, and of those
    clipped = the box was cut by the image's border.  boxes: id -> (x0, x1, y0, y1) of every triangle that has a candidate."""
    W, H = int(cam.W), int(cam.H)
    zn, zf = np.float64(np.float32(cam.z_near)), np.float64(np.float32(cam.z_far))
    out = dict(pix=[], key=[], t=[], Zp=[], Zc=[], corners=[])
    stats = dict(triangles=0, drawn=0, clipped=0, **{k: 0 for k in DROPS})
    boxes, base = {}, 0
    for (conf, pts, _), M in zip(views, matrices):
        conf, pts = np32(conf), np32(pts).reshape(-1, 3)
        tris, dropped = view_triangles(conf, thr)
        stats["conf"] += dropped
        stats["triangles"] += dropped + len(tris)
        Z, u, v = project(compose(cam.w2c, M), cam, pts)
        with np.errstate(all="ignore"):
            xyz = np.isfinite(pts).all(axis=1)
            finite = xyz & np.isfinite(u) & np.isfinite(v)
            near, far = Z >= zn, Z <= zf
            izs = 1.0 / Z
        for i, kind, cs in tris:
            cs = list(cs)
            if not (xyz[cs].all() and np.isfinite(Z[cs]).all()):
                stats["nonfinite"] += 1
                continue
            if not near[cs].all():
                stats["near"] += 1
                continue
            if not far[cs].all():
                stats["far"] += 1
                continue
            if not finite[cs].all():
                stats["nonfinite"] += 1
                continue
            uu, vv, iz = u[cs], v[cs], izs[cs]
            cols, rows = _span(uu.min(), uu.max(), W), _span(vv.min(), vv.max(), H)
            if isinstance(cols, str) or isinstance(rows, str):
                stats["off_image" if "off_image" in (cols, rows) else "no_sample"] += 1
                continue
            tid = 2 * (base + i) + kind
            boxes[tid] = (cols[0], cols[1], rows[0], rows[1])
            stats["drawn"] += 1
            stats["clipped"] += int(cols[2] or rows[2])
            q, r = np.meshgrid(np.arange(cols[0], cols[1] + 1), np.arange(rows[0], rows[1] + 1))
            q, r = q.ravel(), r.ravel()
            px, py = q.astype(np.float64) + 0.5, r.astype(np.float64) + 0.5
            with np.errstate(all="ignore"):
                s0 = _edge(uu[0], vv[0], uu[1], vv[1], px, py)
                s1 = _edge(uu[1], vv[1], uu[2], vv[2], px, py)
                s2 = _edge(uu[2], vv[2], uu[0], vv[0], px, py) if e20 else -_edge(uu[0], vv[0], uu[2], vv[2], px, py)
                den = (s0 + s1) + s2
                if exclusive:
                    inside = ((s0 > 0) & (s1 > 0) & (s2 > 0)) | ((s0 < 0) & (s1 < 0) & (s2 < 0))
                else:
                    inside = ((s0 >= 0) & (s1 >= 0) & (s2 >= 0)) | ((s0 <= 0) & (s1 <= 0) & (s2 <= 0))
                inside &= np.isfinite(den) & (den != 0)
                lam = [s1 / den, s2 / den, s0 / den]
                if affine:
                    t = [lam[0] * np.float64(1.0), lam[1] * np.float64(1.0), lam[2] * np.float64(1.0)]
                    Zp = (lam[0] * (1.0 / iz[0]) + lam[1] * (1.0 / iz[1])) + lam[2] * (1.0 / iz[2])
                else:
                    t = [lam[0] * iz[0], lam[1] * iz[1], lam[2] * iz[2]]
                    Zp = 1.0 / ((t[0] + t[1]) + t[2])
            if affine:
                Zc = np.ones_like(Zp)                                    # colours weighted by lam alone
            else:
                Zc = Zp
            k = inside.nonzero()[0]
            out["pix"].append(r[k].astype(np.int64) * W + q[k])
            out["key"].append((Zp[k].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(tid))
            out["t"].append(np.stack([x[k] for x in t], axis=1))
            out["Zp"].append(Zp[k])
            out["Zc"].append(Zc[k])
            out["corners"].append(np.tile(np.asarray(cs, dtype=np.int64) + base, (len(k), 1)))
        base += conf.size
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dtype=dt)   # noqa: E731
    return dict(pix=cat(out["pix"], (0,), np.int64), key=cat(out["key"], (0,), np.uint64), t=cat(out["t"], (0, 3), np.float64),
                Zp=cat(out["Zp"], (0,), np.float64), Zc=cat(out["Zc"], (0,), np.float64), corners=cat(out["corners"], (0, 3), np.int64), stats=stats, boxes=boxes)


def render(views, matrices, cam, thr, background=(255, 255, 255), **defects):
    """views: list of (conf [H, W], pts [H, W, 3], rgb [H, W, 3]) -> rgb uint8 [H, W, 3], depth fp32 [H, W], index uint32 [H, W] (triangle ids)
    of one camera, and the contenders"""
    W, H = int(cam.W), int(cam.H)
    c = contenders(views, matrices, cam, thr, **defects)
    zbuf = np.full(H * W, EMPTY, dtype=np.uint64)
    np.minimum.at(zbuf, c["pix"], c["key"])
    hit = zbuf != EMPTY
    index = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    depth = (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    depth[~hit] = np.inf
    rgb = np.empty((H * W, 3), dtype=np.uint8)
    rgb[:] = np.asarray(background, dtype=np.uint8)
    # the winner of a pixel is the one contender whose key the minimum kept (ids differ, so keys do)
    win = (c["key"] == zbuf[c["pix"]]).nonzero()[0]
    assert len(win) == int(hit.sum())
    colours = np.concatenate([np32(v[2]).reshape(-1, 3) for v in views]).astype(np.float64)
    t, Zp, cs = c["t"][win], c["Zc"][win], c["corners"][win]
    shade = np.empty((len(win), 3), dtype=np.float32)
    for ch in range(3):
        c0, c1, c2 = (colours[cs[:, k], ch] for k in range(3))
        with np.errstate(all="ignore"):
            shade[:, ch] = (((t[:, 0] * c0 + t[:, 1] * c1) + t[:, 2] * c2) * Zp).astype(np.float32)
    rgb[c["pix"][win]] = quantise(shade)[:, :3]
    return rgb.reshape(H, W, 3), depth.reshape(H, W), index.reshape(H, W), c
