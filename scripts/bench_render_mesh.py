"""The mesh rasteriser (csrc/render_mesh.hip; SceneRenderer.render(mesh=True)) against the point rasteriser on the same tensors, in the same run.  One JSON
line per case (append them to profiles/render_mesh_bench.jsonl; with --lib, a scratch build's lines go to profiles/render_mesh_scratch_builds.jsonl).

Scene: a coherent one -- 200 views of 384 x 512 of one smooth surface (depth 2 + smooth waves) from poses that pan across it, back-projected with each
view's pinhole camera, conf = 1 + exp(randn), threshold 1.05; and one view of it.  Cameras of 512 x 384: one orbit camera, 120 orbit cameras, and 8 `close`
cameras -- view poses pushed three quarters of the way to the surface, where a source quad spans about four target pixels; with one view also 8 `near`
cameras pushed until the surface's nearest parts (depth 1.75 .. 2.25) touch the near plane, where single triangles have boxes of up to the whole image.

  mesh      render(mesh=True): memset of the keys, splat, resolve -- device events around the call
  points1/2 render(point_size=1 / 2) on the same renderer
The three forms alternate inside every round; `rounds` rounds after `warmup`: median, min and max.  covered = share of target pixels that are not
background.  wave_share = share of the drawn triangles whose candidate box exceeds MUST3R_RENDER_MESH_WAVE_AREA, from the same projection as fp64 tensor
expressions, over at most 8 of the cameras.  numpy = the restatement tests/render_mesh_ref.py (a Python iteration per triangle, an array per box) for one
camera on 4 views of 48 x 64, the host baseline.

--lib PATH --tag TEXT: time mesh mode alone with another build of the library (make EXTRA=-DRM_WAVE_AREA=<n> or -DRM_NO_WAVE_PATH, csrc/render_mesh.hip).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
THR = 1.05
W, H = 512, 384
VH, VW, FOCAL = 384, 512, 0.9 * 512


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _emit(rec, f):
    line = json.dumps(rec)
    print(line, flush=True)
    if f:
        f.write(line + "\n")
        f.flush()


def pose(v, V):
    """camera to world of view v: pans along x and turns slightly, always facing the surface"""
    s = (v / max(V - 1, 1) - 0.5) if V > 1 else 0.0
    a = -0.5 * s
    c2w = np.eye(4)
    c2w[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    c2w[:3, 3] = [3.0 * s, 0.2 * np.sin(7 * s), 0.0]
    return c2w


def make_scene(V, vh=VH, vw=VW, focal=FOCAL, device=DEV):
    """-> conf [V, vh, vw], pts [V, vh, vw, 3] (world), rgb, poses: every view sees the surface z = 2 + 0.25 sin(1.3 x) cos(1.1 y) approximately (the depth along
    the ray is evaluated at the ray's crossing of z = 2), so neighbouring pixels are neighbouring surface points"""
    g = torch.Generator(device=device).manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(vh, dtype=torch.float64, device=device), torch.arange(vw, dtype=torch.float64, device=device), indexing="ij")
    rays = torch.stack([(xs + 0.5 - vw / 2) / focal, (ys + 0.5 - vh / 2) / focal, torch.ones_like(xs)], dim=-1)
    pts, poses = [], []
    for v in range(V):
        c2w = pose(v, V)
        Rm, t = torch.as_tensor(c2w[:3, :3], device=device), torch.as_tensor(c2w[:3, 3], device=device)
        d = rays @ Rm.T
        p0 = t + d * ((2.0 - t[2]) / d[..., 2:3])
        z = 2.0 + 0.25 * torch.sin(1.3 * p0[..., 0]) * torch.cos(1.1 * p0[..., 1])
        pts.append((t + d * ((z - t[2]) / d[..., 2])[..., None]).float())
        poses.append(c2w)
    pts = torch.stack(pts)
    conf = 1.0 + torch.exp(torch.randn((V, vh, vw), generator=g, device=device))
    rgb = torch.stack([0.5 + 0.5 * torch.sin(3 * pts[..., 0]), 0.5 + 0.5 * torch.cos(4 * pts[..., 1]), 0.5 + 0.5 * torch.sin(5 * pts[..., 2])], dim=-1)
    return conf, pts, rgb.contiguous(), poses


def close_cameras(Rn, poses, n=8, forward=1.5):
    """view poses pushed `forward` along their optical axis towards the surface at depth about 2: a source quad spans about 2 / (2 - forward) target pixels"""
    cams = []
    for k in range(n):
        c2w = poses[(k * len(poses)) // n].copy()
        c2w[:3, 3] = c2w[:3, 3] + forward * c2w[:3, 2]
        cams.append(Rn.Camera(np.linalg.inv(c2w)[:3], FOCAL, FOCAL, W / 2, H / 2, W, H, 0.01, 100.0))
    return cams


def wave_share(conf, pts, cams, thr, wave_area):
    """share of the drawn triangles (all corners pass, the box holds a sample) whose box exceeds wave_area, by fp64 tensor expressions; identity matrices"""
    drawn = big = 0
    for cam in cams[:8]:
        A = torch.as_tensor(np.asarray(cam.w2c, dtype=np.float64), device=conf.device)
        x, y, z = (pts[..., a].double() for a in range(3))
        X = [((A[a, 0] * x + A[a, 1] * y) + A[a, 2] * z) + A[a, 3] for a in range(3)]
        iz = 1.0 / X[2]
        u, v = cam.fx * (X[0] * iz) + cam.cx, cam.fy * (X[1] * iz) + cam.cy
        ok = (conf >= thr) & torch.isfinite(u) & torch.isfinite(v) & (X[2] >= float(np.float32(cam.z_near))) & (X[2] <= float(np.float32(cam.z_far)))
        del x, y, z, X, iz
        corner = lambda t, dr, dc: t[:, dr:t.shape[1] - 1 + dr, dc:t.shape[2] - 1 + dc]     # noqa: E731
        for kind in ((0, 0), (0, 1), (1, 0)), ((0, 1), (1, 0), (1, 1)):
            good = corner(ok, *kind[0]) & corner(ok, *kind[1]) & corner(ok, *kind[2])
            us, vs = torch.stack([corner(u, *k) for k in kind]), torch.stack([corner(v, *k) for k in kind])
            c0, c1 = torch.ceil(us.amin(0) - 0.5).clamp(min=0), torch.floor(us.amax(0) - 0.5).clamp(max=cam.W - 1)
            r0, r1 = torch.ceil(vs.amin(0) - 0.5).clamp(min=0), torch.floor(vs.amax(0) - 0.5).clamp(max=cam.H - 1)
            good &= (c0 <= c1) & (r0 <= r1)
            area = (c1 - c0 + 1) * (r1 - r0 + 1)
            drawn += int(good.sum())
            big += int((good & (area > wave_area)).sum())
            del us, vs, c0, c1, r0, r1, area, good
    return dict(drawn_triangles=drawn, wave_triangles=big, wave_share=big / max(drawn, 1), cameras_counted=min(len(cams), 8))


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _covered(images):
    return float(np.mean([float((im["index"].view(torch.int32) != -1).float().mean()) for im in images]))


def bench_case(name, V, renderer, tensors, cams, args, f, wave_area):
    forms = {"mesh": lambda: renderer.render(cams, THR, mesh=True)}
    if not args.lib:
        forms["points1"] = lambda: renderer.render(cams, THR, 1)
        forms["points2"] = lambda: renderer.render(cams, THR, 2)
    rec = dict(figure="render_mesh_scratch_build" if args.lib else "render_mesh", cameras_kind=name, views=V, pixels=int(tensors[0].numel()),
               target=[W, H], cameras=len(cams), thr=THR)
    if args.lib:
        rec["build"] = args.tag
    for _ in range(args.warmup):
        for k, fn in forms.items():
            rec[f"{k}_covered"] = _covered(fn())
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            ms[k].append(_events(fn)[0])
    for k in forms:
        rec[f"{k}_ms"] = _stats(ms[k], unit="ms")
    if not args.lib:
        for k in ("points1", "points2"):
            rec[f"mesh_over_{k}_median"] = rec["mesh_ms"]["median"] / rec[f"{k}_ms"]["median"]
        rec.update(wave_share(tensors[0], tensors[1], cams, THR, wave_area))
    _emit(rec, f)


def numpy_baseline(Rn, f):
    import render_mesh_ref as MR
    import render_ref as RR
    conf, pts, rgb, poses = make_scene(4, 48, 64, 0.9 * 64, device="cpu")
    views = [(conf[i].numpy(), pts[i].numpy(), rgb[i].numpy()) for i in range(4)]
    cam = Rn.orbit_box(pts.reshape(-1, 3).min(0).values.numpy(), pts.reshape(-1, 3).max(0).values.numpy(), poses[0], 1, W, H)[0]
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = MR.render(views, RR.identity(4), cam, THR)
        secs.append(time.perf_counter() - t0)
    got = Rn.SceneRenderer(views, None, device=DEV).render([cam], THR, mesh=True)[0]
    same = all(np.array_equal(got[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8)) for k, w in zip(("rgb", "depth", "index"), out[:3]))
    _emit(dict(figure="render_mesh_numpy", views=4, pixels=4 * 48 * 64, triangles=out[3]["stats"]["triangles"], target=[W, H], cameras=1,
               numpy_s=_stats(secs, unit="s"), hip_equals_numpy=bool(same), covered=float((out[2] != 0xFFFFFFFF).mean())), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="*", default=[200, 1])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lib", default=None, help="another build of the library: mesh mode alone is timed")
    ap.add_argument("--tag", default="", help="with --lib: what the build changes")
    ap.add_argument("--only", nargs="*", default=None, help="camera kinds to run: orbit, close, near")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from must3r_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from must3r_amd import render as Rn
    f = open(args.out, "a") if args.out else None
    for V in args.views:
        conf, pts, rgb, poses = make_scene(V)
        flat = pts.reshape(-1, 3)
        orbit = Rn.orbit_box(flat.min(0).values.cpu().numpy(), flat.max(0).values.cpu().numpy(), poses[0], 120, W, H)
        renderer = Rn.SceneRenderer([(conf[i], pts[i], rgb[i]) for i in range(V)], None, device=DEV)
        cases = [("orbit", orbit[:1]), ("orbit", orbit), ("close", close_cameras(Rn, poses))]
        if V == 1:
            # the surface's nearest parts reach the camera: corners just beyond the near plane, boxes of up to the whole image
            cases.append(("near", close_cameras(Rn, poses, forward=1.74)))
        for name, cams in cases:
            if args.only is None or name in args.only:
                bench_case(name, V, renderer, (conf, pts, rgb), cams, args, f, _lib.RENDER_MESH_WAVE_AREA)
        del renderer, conf, pts, rgb
        torch.cuda.empty_cache()
    if not args.lib and not args.no_numpy:
        numpy_baseline(Rn, f)


if __name__ == "__main__":
    main()
