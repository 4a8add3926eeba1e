"""The keyframe map's 1-NN index (csrc/nn_index.hip; must3r_amd.slam_nn.BVH_hip / BVHQuadrant_hip) against the brute force, and the
video modes end to end.  One JSON line per figure (append them to profiles/nn_index_bench.jsonl):

  (a) query: 49 152 queries (one 384 x 512 frame at subsample 2) against maps of 10 / 50 / 100 / 200 keyframes of
      synthetic.make_overlap_frames at 384 x 512 (each keyframe adds its points of conf > 1.5 at subsample 2, as
      demo.slam_update_scene_state does), queried with the next frame (frames[n_kf]: it overlaps the latest keyframes, as in
      vidslam): the index vs QuandrantSearcher (both quadrant_x2), and the plain index vs nn_distances; leaf sizes 16 / 32 / 64
      (NN_LEAF_LOG2) at 8 lanes per query, and 1 / 4 / 8 / 16 lanes per query (NN_QUERY_LANES_LOG2) at leaves of 32
  (b) rebuild of the index at the same map sizes (quadrant_x2 and plain)
  (c) frames per second of demo.must3r_inference_video on a 200-frame 384 x 512 PNG sequence with the MUSt3R_512 geometry (synthetic
      weights): vidseq, vidslam on the brute-force searcher, vidslam on the index; keyframes and map size of the vidslam runs

Timings are device events around `reps` calls after `warmup` calls, repeated `rounds` times: median, min and max of the rounds.
Kernel names and per-kernel times: run with --skip-video under `rocprofv3 --kernel-trace --stats` (a separate run).
"""
import argparse
import functools
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from must3r_amd import _lib  # noqa: E402
from must3r_amd import synthetic as S  # noqa: E402
from must3r_amd.slam_nn import BVH_hip, BruteForce_hip, QuandrantSearcher, get_searcher, nn_distances  # noqa: E402

DEV = "cuda:0"


def _timed(fn, warmup, reps, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return dict(ms_median=float(np.median(out)), ms_min=float(min(out)), ms_max=float(max(out)), warmup=warmup, reps=reps, rounds=rounds)


def _emit(rec, f):
    line = json.dumps(rec)
    print(line, flush=True)
    if f:
        f.write(line + "\n")
        f.flush()


def bench_map(args, f):
    frames = S.make_overlap_frames(0, n_kf=max(args.keyframes), H=384, W=512)
    kf = []
    for fr in frames[:-1]:
        sel = fr["pts3d"][0, 0, ::2, ::2][fr["conf"][0, 0, ::2, ::2] > 1.5]
        kf.append((torch.from_numpy(np.ascontiguousarray(sel)).to(DEV), torch.from_numpy(fr["cam"])))
    for n_kf in args.keyframes:
        nxt = frames[n_kf]      # the frame after the map's last keyframe: it overlaps the latest keyframes, as a vidslam query does
        q = torch.from_numpy(np.ascontiguousarray(nxt["pts3d"][0, 0, ::2, ::2].reshape(-1, 3))).to(DEV)
        cam = torch.from_numpy(nxt["cam"])
        brute_q, brute_p = QuandrantSearcher("kdtree-scipy-quadrant_x2"), BruteForce_hip()
        for p, c in kf[:n_kf]:
            brute_q.add_pts(p, cam_center=c)
            brute_p.add_pts(p)
        n = brute_p.n
        db = brute_p.all_points[:n]
        ref_q = brute_q.query_device(q, cam_center=cam)
        ref_p = nn_distances(db, q)
        rec = dict(figure="query", keyframes=n_kf, query_frame=n_kf, map_points=n, queries=int(q.shape[0]),
                   median_nn_distance=float(ref_p.median()),
                   brute_quadrant_x2=_timed(lambda: brute_q.query_device(q, cam_center=cam), args.warmup, args.reps, args.rounds),
                   brute_plain=_timed(lambda: nn_distances(db, q), args.warmup, args.reps, args.rounds))
        # leaf sizes at the default lanes per query, then lanes per query at the default leaf size
        for leaf_log2, lanes_log2 in ((4, 3), (5, 3), (6, 3), (5, 0), (5, 2), (5, 4)):
            _lib.set_option("NN_LEAF_LOG2", leaf_log2)
            _lib.set_option("NN_QUERY_LANES_LOG2", lanes_log2)
            idx_q, idx_p = get_searcher("bvh-hip-quadrant_x2"), BVH_hip()
            for p, c in kf[:n_kf]:
                idx_q.add_pts(p, cam_center=c)
                idx_p.add_pts(p)
            assert torch.equal(idx_q.query_device(q, cam_center=cam), ref_q) and torch.equal(idx_p.query_device(q), ref_p)
            tag = f"L{1 << leaf_log2}_G{1 << lanes_log2}"
            rec[f"index_quadrant_x2_{tag}"] = _timed(lambda: idx_q.query_device(q, cam_center=cam), args.warmup, args.reps, args.rounds)
            rec[f"index_plain_{tag}"] = _timed(lambda: idx_p.query_device(q), args.warmup, args.reps, args.rounds)
            if lanes_log2 == 3:
                rec[f"rebuild_quadrant_x2_L{1 << leaf_log2}"] = _timed(idx_q.build, args.warmup, max(1, args.reps // 4), args.rounds)
                rec[f"rebuild_plain_L{1 << leaf_log2}"] = _timed(idx_p.build, args.warmup, max(1, args.reps // 4), args.rounds)
        _lib.set_option("NN_LEAF_LOG2", 5)
        _lib.set_option("NN_QUERY_LANES_LOG2", 3)
        rec["speedup_quadrant_x2_default"] = rec["brute_quadrant_x2"]["ms_median"] / rec["index_quadrant_x2_L32_G8"]["ms_median"]
        rec["speedup_plain_default"] = rec["brute_plain"]["ms_median"] / rec["index_plain_L32_G8"]["ms_median"]
        rec["bound"] = ("index query: latency of the dependent node and leaf loads of each walk (one walk per query, shared by G lanes); "
                        "brute force: fp32 VALU; rebuild: launch and memory latency (4 x 3 radix passes + one launch per tree level)")
        _emit(rec, f)


def bench_video(args, f):
    import PIL.Image
    from bench import build_models
    from must3r_amd import demo as Dm
    from must3r_amd.config import MUST3R_512
    enc, dec, _, _ = build_models(MUST3R_512, "fp16wa", DEV)
    tmp = tempfile.mkdtemp(prefix="nn_index_video_")
    g = np.random.default_rng(0)
    base = g.integers(0, 256, (40, 60, 3)).astype(np.uint8)
    big = np.asarray(PIL.Image.fromarray(base).resize((900, 600), PIL.Image.BILINEAR))
    files = []
    for i in range(args.frames):            # a slow pan over one textured image: consecutive frames overlap
        x0 = int(i * (900 - 512) / max(1, args.frames - 1))
        p = os.path.join(tmp, f"frame{i:04d}.png")
        PIL.Image.fromarray(np.ascontiguousarray(big[100:484, x0:x0 + 512])).save(p)
        files.append(p)
    runs = [("vidseq", None), ("vidslam", "kdtree-scipy-quadrant_x2"), ("vidslam", "bvh-hip-quadrant_x2")]
    for rep in range(args.video_rounds + 1):    # round 0 is the warm-up
        for mode, method in runs:
            flags = []
            tree = None
            if method and method.startswith("bvh"):
                tree = get_searcher(method)
            elif method:
                class OnDevice(QuandrantSearcher):   # the driver's results are on the host; the brute force takes device points
                    def add_pts(self, pts, cam_center, **kw):
                        super().add_pts(pts.to(DEV), cam_center)

                    def query(self, pts, cam_center, **kw):
                        return super().query(pts.to(DEV), cam_center)
                tree = OnDevice(method)
            if mode == "vidseq":
                key = lambda id, res, scene_state: id % 5 == 0   # noqa: E731
                upd = lambda res, scene_state: scene_state      # noqa: E731
                lcs = 25
            else:
                inner = functools.partial(Dm.slam_is_keyframe, 2, 1.5, args.overlap_thr, 70, "nn-norm")

                def key(id, res, scene_state, inner=inner):
                    flags.append(bool(inner(id, res, scene_state)))
                    return flags[-1]
                upd = functools.partial(Dm.slam_update_scene_state, 2, 1.5)
                lcs = 25
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scene = Dm.must3r_inference_video((enc, dec), DEV, 512, "fp16", files, 0, 2, 1, local_context_size=lcs, is_keyframe_function=key,
                                              scene_state=tree, scene_state_update_function=upd, verbose=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep == 0:
                continue
            rec = dict(figure="video", mode=mode, searcher=method, frames=len(files), round=rep, seconds=dt, fps=len(files) / dt,
                       keyframes=None if mode == "vidseq" else 2 + sum(flags),
                       map_points=None if tree is None else (tree.n if isinstance(tree, BVH_hip) else
                                                              sum(s.n for s in tree.search_structs)),
                       note="end to end: PNG decode and resize, encoder, decoder, postprocess(compute_cam), keyframe test, host copies")
            _emit(rec, f)
            del scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[10, 50, 100, 200])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--video-rounds", type=int, default=2)
    ap.add_argument("--overlap-thr", type=float, default=0.05)
    ap.add_argument("--skip-video", action="store_true")
    ap.add_argument("--skip-map", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    f = open(args.out, "a") if args.out else None
    if not args.skip_map:
        bench_map(args, f)
    if not args.skip_video:
        bench_video(args, f)


if __name__ == "__main__":
    main()
