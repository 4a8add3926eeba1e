"""The SLAM agent's per-frame step (csrc/slam.hip, must3r_amd/slam.py) beside the composed form it replaces, on one GPU in one run.  One JSON line per run
(append it to profiles/slam_bench.jsonl).  Not run by the tests; bench.py is left alone.

  (a) the step alone: one frame of ``--height`` x ``--width`` (384 x 512) raw head output, ``subsamp`` 2 and 4, against a fixed map of ``--map-points``
      points (0.4 M and 3.7 M, the sizes of profiles/nn_index_bench.jsonl) in a quadrant_x2 index.  NEW: must3r_hip_slam_pose + must3r_hip_slam_keyframe +
      the one read of the record.  COMPOSED: engine.postprocess, get_camera_pose as torch expressions on the device (the Weiszfeld loop and the weighted
      Procrustes of oracle/cam_ref.py, with the in-place rectification), slam_nn.get_overlap_score on the same searcher, the median and the focal reads of
      demo.slam_is_keyframe / MUSt3R_Agent.update.  The two forms alternate inside every round; wall time including the reads.
  (b) the loop: ``--frames`` synthetic frames through SLAM_MUSt3R at the released geometry with random-init weights, frames/s and keyframes, with the
      decision as computed and with the decision scripted to every third frame; the composed form in the same loop (``ComposedAgent``).

Timings: ``--warmup`` runs, then ``--rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared: the record says so."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from must3r_amd import slam, synthetic as S  # noqa: E402
from must3r_amd.engine import postprocess  # noqa: E402
from must3r_amd.slam_nn import BVHQuadrant_hip, get_overlap_score  # noqa: E402
from oracle import cam_ref  # noqa: E402

DEV = "cuda:0"


def _stats(xs, **kw):
    return dict(median_ms=float(np.median(xs)) * 1e3, min_ms=float(min(xs)) * 1e3, max_ms=float(max(xs)) * 1e3, rounds=len(xs), **kw)


def torch_camera_pose(res, seq_focal, HW, is_first_frame=False):
    """slam/model.py:147-172 as torch expressions on the device of ``res`` (the composed form's pose)"""
    H, W = HW
    dev = res["pts3d"].device
    B = res["pts3d"].shape[1]
    pix = cam_ref.xy_grid(W, H, device=dev).view(1, -1, 2) - torch.tensor((W / 2, H / 2), device=dev).view(-1, 1, 2)
    pts = res["pts3d_local"][0].flatten(1, 2)
    q = (pts[..., :2] / pts[..., 2:3]).nan_to_num(posinf=0, neginf=0)
    a, b = (q * pix).sum(-1), q.square().sum(-1)
    focal = a.mean(1) / b.mean(1)
    for _ in range(10):
        w = (pix - focal.view(-1, 1, 1) * q).norm(dim=-1).clip(min=1e-8).reciprocal()
        focal = (w * a).mean(1) / (w * b).mean(1)
    c2w = torch.eye(4, device=dev).repeat(B, 1, 1)
    if not is_first_frame:
        local = res["pts3d_local"][0].view(B, -1, 3)
        if seq_focal is not None:
            local[..., -1] *= seq_focal / focal[:, None]
        R, T = cam_ref.rigid_points_registration(local, res["pts3d"][0].view(B, -1, 3), weights=res["conf"][0].view(B, -1) - 1.0)
        c2w[:, :3, :3], c2w[:, :3, 3] = R, T
    return c2w, focal


def composed_step(raw, H, W, tree, seq, is_first, cfg):
    """the per-frame step as the package composed it before: every read the issue lists is here"""
    res = postprocess(raw.reshape(1, 1, H, W, 7))
    c2w, focal = torch_camera_pose(res, slam.mean_focal(seq), (H, W), is_first)
    cam_center = c2w[0, :3, -1]
    score = get_overlap_score(res, tree, cam_center, mode="nn-norm", kf_x_subsamp=cfg["subsamp"], min_conf_keyframe=cfg["min_conf"], percentile=cfg["percentile"])
    conf = res["conf"][0, 0]
    iskf = bool(is_first or (score > cfg["thr"] and conf.median() > cfg["min_conf"]))
    seq["f"].append(float(focal[0].cpu()))
    seq["conf"].append(float(conf.mean().cpu()) - 1.0)
    s = cfg["subsamp"]
    msk = conf[::s, ::s] > cfg["min_conf"]
    return res, c2w[0], cam_center, res["pts3d"][0, 0, ::s, ::s][msk], iskf, score


def native_step(raw, H, W, tree, state, is_first, cfg):
    out = slam.slam_pose(raw.reshape(1, H, W, 7), seq_focals=state, is_first_frame=is_first, update_focal=True)
    sel, record, _ = slam.slam_keyframe(out["pts3d"][0], out["pts3d_local"][0], out["conf"][0], out["c2w"][0], tree, "nn-norm", cfg["subsamp"],
                                        cfg["min_conf"], cfg["percentile"], out["focal"], state)
    rec = slam.read_record(record)
    return rec


def bench_step(args):
    H, W = args.height, args.width
    raw = S.make_cam_pointmaps(1, H, W, focal=0.9 * W, noise=0.02, seed=1).to(DEV)
    act = postprocess(raw)
    centre = torch.zeros(3)
    out = {}
    for n_map in args.map_points:
        g = torch.Generator().manual_seed(n_map)
        # a map around the frame's own points: the frame overlaps the map, as in a running agent
        base = act["pts3d"].reshape(-1, 3).cpu()
        pts = base[torch.randint(0, base.shape[0], (n_map,), generator=g)] + 0.05 * torch.randn(n_map, 3, generator=g)
        tree = BVHQuadrant_hip("bvh-hip-quadrant_x2")
        tree.add_pts(pts.to(DEV), cam_center=centre)
        tree.build()
        for sub in (2, 4):
            cfg = dict(subsamp=sub, min_conf=1.2, percentile=85.0, thr=0.1)
            state = slam.FocalState()
            native_step(raw, H, W, tree, state, True, cfg)
            f0, c0 = state.read()   # the composed form starts from the same running focal as the new one
            seq = {"f": [float(f0[0])], "conf": [float(c0[0])]}
            times = {"new": [], "composed": []}
            scores = {}
            for r in range(args.warmup + args.rounds):
                for form in ("new", "composed"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if form == "new":
                        scores[form] = float(native_step(raw, H, W, tree, state, False, cfg)[slam.REC["score"]])
                    else:
                        seq_r = {"f": list(seq["f"]), "conf": list(seq["conf"])}
                        scores[form] = float(composed_step(raw, H, W, tree, seq_r, False, cfg)[5])
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        times[form].append(time.perf_counter() - t0)
            out[f"map{n_map}_sub{sub}"] = dict(new=_stats(times["new"], score=scores["new"]), composed=_stats(times["composed"], score=scores["composed"]),
                                               candidates=slam.candidates(H, W, sub))
    return out


class ComposedAgent(slam.SLAM_MUSt3R):
    """the loop with the composed per-frame step"""

    def __init__(self, *a, cfg=None, **k):
        self.cfg, self.seq = cfg, {"f": [], "conf": []}
        super().__init__(*a, **k)

    def reset(self):
        super().reset()
        self.seq = {"f": [], "conf": []}

    def frame_step(self, agent, view, pred, is_first_frame, to_orig_focal):
        H, W = (int(v) for v in view["true_shape"][0])
        res, c2w, cam, sel, iskf, score = composed_step(pred["pointmaps"], H, W, self.overlap_tree, self.seq, is_first_frame, self.cfg)
        rec = np.zeros(32)
        rec[slam.REC["c2w"]] = c2w.double().cpu().numpy().reshape(-1)
        rec[slam.REC["conf_mean"]] = self.seq["conf"][-1] + 1.0
        return sel, res["pts3d"][0, 0], None, res["pts3d_local"][0, 0, ..., -1], res["conf"][0, 0], slam.mean_focal(self.seq), slam.rigid_inverse(c2w), cam, iskf, rec


def bench_loop(args):
    import must3r_amd.model as M
    from must3r_amd.config import MUST3R_512 as cfg
    enc = M.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads)
    dec = M.MUSt3R(img_size=(cfg.img_size,) * 2, enc_embed_dim=cfg.enc_dim, embed_dim=cfg.dec_dim, depth=cfg.dec_depth, num_heads=cfg.dec_heads,
                   feedback_type="single_mlp", memory_mode="kv")
    enc.load_state_dict(S.make_encoder_state_dict(cfg, 0))
    dec.load_state_dict(S.make_decoder_state_dict(cfg, 0))
    model = (enc.to(DEV).eval(), dec.to(DEV).eval())
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:384, 0:512].astype(np.float32)
    frames = [np.clip(127 + 90 * np.stack([np.sin(0.02 * xx + 0.1 * t), np.cos(0.03 * yy - 0.07 * t), np.sin(0.01 * (xx + yy) + 0.2 * t)], -1)
                      + 20 * rng.standard_normal((384, 512, 3)), 0, 255).astype(np.uint8) for t in range(args.frames)]
    step = dict(subsamp=2, min_conf=1.2, percentile=85.0, thr=0.1)
    out = {}
    for scripted in (False, True):
        for form in ("new", "composed"):
            kw = dict(res=512, kf_x_subsamp=2, keyframe_overlap_thr=0.1, min_conf_keyframe=1.2, overlap_percentile=85.0, device=DEV)
            agent = slam.SLAM_MUSt3R(model, **kw) if form == "new" else ComposedAgent(model, cfg=step, **kw)
            if scripted:   # the decision scripted to every third frame: both forms do identical work
                inner = agent.frame_step

                def scripted_step(ag, view, pred, is_first, to_orig, inner=inner):
                    r = list(inner(ag, view, pred, is_first, to_orig))
                    r[8] = bool(is_first or int(view["idx"]) % 3 == 0)
                    return tuple(r)
                agent.frame_step = scripted_step
            for img in frames[:3]:
                agent(img, 0, 0, device_outputs=True)   # warm-up
            agent.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t, img in enumerate(frames):
                agent(img, t, 0, device_outputs=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[f"{form}_{'scripted' if scripted else 'free'}"] = dict(frames_per_s=len(frames) / dt, keyframes=len(agent.keyframes),
                                                                       map_points=0 if agent.overlap_tree is None else int(agent.overlap_tree.n))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--map-points", type=int, nargs="+", default=[400_000, 3_700_000])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = dict(bench="slam", device=torch.cuda.get_device_name(0), clocks="not pinned, shared machine", step=bench_step(args))
    if not args.skip_loop:
        rec["loop"] = bench_loop(args)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
