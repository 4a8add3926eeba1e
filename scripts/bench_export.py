"""Scene export (csrc/export.hip; must3r_amd.export, demo.export_scene_thresholds) against the numpy restatement of the reference's
method (tests/export_ref.py: boolean mask, concatenate, fp64 transform, once per threshold).  One JSON line per figure (append them to
profiles/export_bench.jsonl).  Sizes: point cloud at 20 and 200 views of 384 x 512, mesh at 20 views; the reference's eight thresholds.

  (a) kernels: count + scan + the eight scatters (mesh: + the vertex planes), device events, useful bytes moved (conf once for the
      count and once per scatter, 24 B read + 16 B written per selected point, 12 B per face) and their fraction of 6.3 TB/s
  (b) files: demo.export_scene_thresholds to eight files on disk from a device-resident scene and from a host-resident scene (upload
      included), wall clock, beside the yardstick writing the same eight files (byte-identical, checked) from the restatement's arrays
      through the same containers.  The yardstick is the reference's method, never the code under test.

Timings: `warmup` runs, then `rounds` rounds: median, min and max.  Per-kernel times: run with --kernels-only under
`rocprofv3 --kernel-trace --stats` (a separate run; profiles/export_kernel_stats.txt).
"""
import argparse
import filecmp
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import export_ref as R  # noqa: E402
from must3r_amd import _lib, demo as Dm, export as E  # noqa: E402

DEV = "cuda:0"
THR = list(E.REFERENCE_THRESHOLDS)
HBM_BYTES_PER_S = 6.3e12


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _emit(rec, f):
    line = json.dumps(rec)
    print(line, flush=True)
    if f:
        f.write(line + "\n")
        f.flush()


def make_scene(V, H, W, device):
    """seeded: points in front of a slowly moving camera, conf = 1 + exp(randn), colours in [0, 1]; host scene = the device scene's copy"""
    g = torch.Generator(device=DEV).manual_seed(0)
    x_out, imgs, cams = [], [], []
    for i in range(V):
        conf = 1.0 + torch.exp(torch.randn((H, W), generator=g, device=DEV))
        pts = torch.randn((H, W, 3), generator=g, device=DEV)
        rgb = torch.rand((H, W, 3), generator=g, device=DEV)
        c2w = torch.eye(4)
        c2w[:3, 3] = torch.tensor([0.01 * i, 0.0, 0.02 * i])
        if device is None:
            conf, pts, rgb = conf.cpu(), pts.cpu(), rgb.cpu().numpy()
        x_out.append(dict(conf=conf, pts3d=pts, c2w=c2w))
        imgs.append(rgb)
        cams.append(c2w)
    return R.FakeScene(x_out, imgs, [300.0] * V, cams)


def bench_kernels(scene, mesh, args):
    S, M = E.view_matrices(scene.cams2world, False)
    ex = E.SceneExporter(E.scene_views(scene), M)
    n_pix = ex.n_pix

    def run():
        totals = ex.count(THR, mesh=mesh)
        if mesh:
            dev, _ = ex._buffers(16 * n_pix)
            _lib.check(ex.lib.must3r_hip_export_vertices(ex.table, ex.n, len(THR), ex.scratch.data_ptr(), dev.data_ptr(), dev.data_ptr() + 12 * n_pix,
                                                         ex._minmax.data_ptr(), ex._stream()))
            for k in range(len(THR)):
                ex.faces_device(k)
        else:
            for k in range(len(THR)):
                ex.points_device(k, _lib.EXPORT_GLB)
        return totals

    for _ in range(args.warmup):
        totals = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    if mesh:
        nbytes = 4 * n_pix + 40 * n_pix + sum(4 * n_pix + 12 * t for t in totals)
    else:
        nbytes = 4 * n_pix + sum(4 * n_pix + 40 * t for t in totals)
    st = _stats(ms, unit="ms")
    return dict(totals=totals, bytes=int(nbytes), ms=st, fraction_of_6p3_TBps=nbytes / (st["median"] * 1e-3) / HBM_BYTES_PER_S)


def yardstick(outdir, scene, mesh):
    """the reference's method in numpy, once per threshold, written through the same containers"""
    views, M = R.scene_views(scene), R.view_matrices(scene.cams2world, False)
    S = R.scene_transform(scene.cams2world[0])
    cams = E.camera_frustums(scene, S, 0.05, [bool(np.median(v[0]) >= 0.0) for v in views])
    os.makedirs(outdir, exist_ok=True)
    paths = []
    for thr in THR:
        path = os.path.join(outdir, f"scene_{thr}.glb")
        if mesh:
            pos, col, faces = R.mesh(views, M, thr)
            E.write_glb(path, pos, col, pos.min(0), pos.max(0), faces=faces, cameras=cams)
        else:
            pos, col = R.pointcloud(views, M, thr)
            E.write_glb(path, pos, col, pos.min(0), pos.max(0), cameras=cams)
        paths.append(path)
    return paths


def _wall(fn, rounds, cleanup):
    out = []
    for _ in range(rounds):
        cleanup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def bench_size(V, mesh, args, f):
    H, W = 384, 512
    dev_scene, host_scene = make_scene(V, H, W, DEV), make_scene(V, H, W, None)
    tmp = tempfile.mkdtemp(prefix="export_bench_", dir=args.tmp)
    d_dev, d_host, d_ref = (os.path.join(tmp, n) for n in ("dev", "host", "ref"))
    kw = dict(file_type="glb", as_pointcloud=not mesh)
    try:
        rec = dict(figure="export", kind="mesh" if mesh else "pointcloud", views=V, H=H, W=W, pixels=V * H * W, thresholds=THR,
                   threads=torch.get_num_threads())
        rec["kernels"] = bench_kernels(dev_scene, mesh, args)
        if args.kernels_only:
            _emit(rec, f)
            return
        # byte identity of the three routes, once
        a = Dm.export_scene_thresholds(d_dev, dev_scene, THR, **kw)
        b = Dm.export_scene_thresholds(d_host, host_scene, THR, **kw)
        c = yardstick(d_ref, host_scene, mesh)
        assert len(a) == len(b) == len(c) == len(THR)
        assert all(filecmp.cmp(x, y, shallow=False) and filecmp.cmp(x, z, shallow=False) for x, y, z in zip(a, b, c))
        rec["file_bytes"] = int(sum(os.path.getsize(p) for p in a))
        rec["identical_files"] = True

        def clean():
            for d in (d_dev, d_host, d_ref):
                shutil.rmtree(d, ignore_errors=True)
        rec["device_resident_s"] = _stats(_wall(lambda: Dm.export_scene_thresholds(d_dev, dev_scene, THR, **kw), args.rounds, clean), unit="s")
        rec["host_resident_s"] = _stats(_wall(lambda: Dm.export_scene_thresholds(d_host, host_scene, THR, **kw), args.rounds, clean), unit="s")
        rec["yardstick_numpy_s"] = _stats(_wall(lambda: yardstick(d_ref, host_scene, mesh), args.yardstick_rounds, clean), unit="s")
        rec["speedup_device_resident_min"] = rec["yardstick_numpy_s"]["min"] / rec["device_resident_s"]["min"]
        rec["speedup_host_resident_min"] = rec["yardstick_numpy_s"]["min"] / rec["host_resident_s"]["min"]
        rec["gate_device_resident_below_yardstick"] = rec["device_resident_s"]["min"] < rec["yardstick_numpy_s"]["min"]
        _emit(rec, f)
        assert rec["gate_device_resident_below_yardstick"], rec
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pointcloud-views", type=int, nargs="*", default=[20, 200])
    ap.add_argument("--mesh-views", type=int, nargs="*", default=[20])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--yardstick-rounds", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="figure (a) alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--tmp", default=None, help="directory for the exported files (default: the system's temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    f = open(args.out, "a") if args.out else None
    for V in args.pointcloud_views:
        bench_size(V, False, args, f)
    for V in args.mesh_views:
        bench_size(V, True, args, f)


if __name__ == "__main__":
    main()
